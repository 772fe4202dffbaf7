"""Independent references for the five gfx950 kernels of
native/src/health/liveness_kernel.hip, and the comparisons the raw-output
tests apply to what the kernels wrote.

Pure Python ints and numpy; nothing native is imported. Written from the
contract stated in liveness_kernel.h (operand formulas, record words, argument
structs) and the MFMA register layouts of cdna_hip_programming.md section 3,
not from the host verifiers: those share probe_a/b/c with the kernels, so
they can only agree with themselves.

All generator arithmetic is unsigned 32-bit: `i*3u + k*5u + nonce` wraps, and
7, 5 and 4 do not all divide 2^32, so a reference that forgets the wrap
differs near nonce 2^32 (0xFFFFFFF9 is in NONCES for that reason).
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

PROBE_M = PROBE_N = 32
PROBE_K = 2
PROBE_MAGIC = 0x4D464D41   # "MFMA"
SWEEP_MAGIC = 0x43484950   # "CHIP"
PERF_MAGIC = 0x50455246    # "PERF"
SWEEP_LDS_WORDS = 40960 - 16
SCRATCH_FLOATS = 16 * 64
REC_WORDS = 16
NUM_XCC_MAX = 8            # an MI355X has 8 XCDs; a partition has fewer

# liveness meta words
META_MAGIC, META_NONCE, META_XCC, META_HWID = 0, 1, 2, 3
# chip-sweep record words
REC_MAGIC, REC_NONCE, REC_XCC, REC_HWID, REC_MFMA_BAD, REC_LDS_BAD, REC_ARRIVED = 0, 1, 2, 3, 4, 5, 6
REC_T0_LO, REC_T0_HI, REC_T1_LO, REC_T1_HI, REC_WG = 7, 8, 9, 10, 11
# mfma-burn record words
PREC_MAGIC, PREC_WG, PREC_XCC, PREC_HWID = 0, 1, 2, 3
PREC_RT0_LO, PREC_RT0_HI, PREC_RT1_LO, PREC_RT1_HI, PREC_CYC_LO, PREC_CYC_HI, PREC_NONCE, PREC_SUM = 4, 5, 6, 7, 8, 9, 10, 12

NONCES = (0, 1, 6, 7, 34, 35, 12345, 0xDEADBEEF, 0xFFFFFFF9, 0xFFFFFFFF)
ITERS = (1, 4, 64, 1 << 20)
BURN_NONCES = (0, 1, 0xDEADBEEF, 0xFFFFFFFF)
BURN_ITERS = (1, 2, 3)


# ---- operand generators (mod 2^32) -------------------------------------------
def probe_a(i: int, k: int, nonce: int) -> int:
    return ((i * 3 + k * 5 + nonce) & M32) % 7 - 3


def probe_b(k: int, j: int, nonce: int) -> int:
    return ((j * 11 + k * 2 + nonce) & M32) % 5 - 2


def probe_c(i: int, j: int, nonce: int) -> int:
    return ((i + 2 * j + nonce) & M32) % 4


def sweep_nonce(nonce: int, wg: int, wave: int) -> int:
    return (nonce + wg * 4 + wave) & M32


def sweep_lds_pattern(i: int, nonce: int, wg: int) -> int:
    return ((i * 2654435761) & M32) ^ ((nonce + wg * 0x9E3779B1) & M32)


def hbm_pattern(word: int, seed: int) -> int:
    """32-bit word `word` (a 64-bit index) of the patterned buffer: the high
    half of the index is folded into the low half before the multiply."""
    return ((((word ^ (word >> 32)) & M32) * 0x9E3779B1) + seed) & M32


def hbm_pattern_words(count: int, seed: int, first: int = 0) -> np.ndarray:
    """hbm_pattern of `count` consecutive words as a uint32 array."""
    w = np.arange(first, first + count, dtype=np.uint64)
    x = (w ^ (w >> np.uint64(32))) & np.uint64(M32)
    return ((x * np.uint64(0x9E3779B1) + np.uint64(seed)) & np.uint64(M32)).astype(np.uint32)


def burn_bf16_bits(lane: int, j: int, nonce: int) -> int:
    h = ((lane * 0x9E3779B1) & M32) ^ ((j * 0x85EBCA77) & M32) ^ nonce
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    h ^= h >> 12
    return (h & 0x807F) | ((120 + (h >> 8) % 7) << 7)


def bf16_value(bits: int) -> float:
    """The value of a bf16 bit pattern: a float32 whose low 16 bits are zero."""
    return float(np.array([bits << 16], dtype=np.uint32).view(np.float32)[0])


# ---- f32 tile (mi355x_mfma_liveness, mi355x_chip_sweep) ------------------------
def tile_operands(nonce: int):
    a = np.array([[probe_a(i, k, nonce) for k in range(PROBE_K)] for i in range(PROBE_M)], dtype=np.int64)
    b = np.array([[probe_b(k, j, nonce) for j in range(PROBE_N)] for k in range(PROBE_K)], dtype=np.int64)
    c = np.array([[probe_c(i, j, nonce) for j in range(PROBE_N)] for i in range(PROBE_M)], dtype=np.int64)
    return a, b, c


def tile(nonce: int, iters: int) -> np.ndarray:
    """The exact 32x32 result C + iters * A.B, int64."""
    a, b, c = tile_operands(nonce)
    return c + iters * (a @ b)


def tile_f32(nonce: int, iters: int) -> np.ndarray:
    t = tile(nonce, iters)
    assert np.abs(t).max() < 1 << 24      # so every partial sum is an exact fp32 number
    return t.astype(np.float32)


# ---- how many iterations the tile stays exact for (MI355X_PROBE_MAX_ITERS) -----
PROBE_MAX_ITERS = 1398101
# Every nonce class there is: without a wrap the operands depend on nonce mod
# lcm(4, 7, 5) = 140; the largest index term is 11*31 + 2 = 343, so each nonce
# from 2^32 - 343 on wraps in its own set of terms and is listed itself.
TRIPLE_NONCES = tuple(range(280)) + tuple(range((1 << 32) - 1024, 1 << 32))


def operand_triples(nonces=TRIPLE_NONCES) -> dict:
    """Every (c, a0*b0, a1*b1) an element of the tile can have, each with one
    (nonce, i, j) that produces it. Integer arithmetic mod 2^32, like the header's."""
    found = {}
    i = np.arange(PROBE_M, dtype=np.uint64)[:, None]
    j = np.arange(PROBE_N, dtype=np.uint64)[None, :]
    m32 = np.uint64(M32)
    for n in nonces:
        n64 = np.uint64(n)
        a = [(((i * np.uint64(3) + np.uint64(5 * k) + n64) & m32) % np.uint64(7)).astype(np.int64) - 3 for k in (0, 1)]
        b = [(((j * np.uint64(11) + np.uint64(2 * k) + n64) & m32) % np.uint64(5)).astype(np.int64) - 2 for k in (0, 1)]
        c = (((i + np.uint64(2) * j + n64) & m32) % np.uint64(4)).astype(np.int64)
        packed = (c * 64 + (a[0] * b[0] + 8)) * 64 + (a[1] * b[1] + 8)      # products lie in -6..6
        values, first = np.unique(packed.ravel(), return_index=True)
        for v, at in zip(values.tolist(), first.tolist()):
            found.setdefault((v // 4096, v // 64 % 64 - 8, v % 64 - 8), (n, at // PROBE_N, at % PROBE_N))
    return found


def fp32_holds(v: int) -> bool:
    """Whether fp32 represents the integer v exactly (24 significant bits)."""
    v = abs(v)
    return v == 0 or (v >> ((v & -v).bit_length() - 1)).bit_length() <= 24


def inexact_steps(triple, iters: int) -> list:
    """The values of one element's computation over `iters` iterations that fp32
    does not hold exactly: the accumulator after every product, with the two
    products of an iteration in either order, and the host's float(iters) * dot
    and c + float(iters) * dot. Each is linear in the iteration number, so its
    magnitude is largest at an end, and the first iteration's values are tiny:
    the iterations are walked from the last one down until all of one
    iteration's values are at most 2^24 in magnitude; every value before that is
    an integer below 2^24, which fp32 holds."""
    c, p0, p1 = triple
    dot = p0 + p1
    assert max(abs(c), abs(c + p0), abs(c + p1), abs(c + dot)) < 1 << 24
    bad = [v for v in (iters * dot, c + iters * dot) if not fp32_holds(v)]
    for t in reversed(range(iters)):
        values = (c + t * dot + p0, c + t * dot + p1, c + (t + 1) * dot)
        if all(abs(v) <= 1 << 24 for v in values):
            break
        bad += [v for v in values if not fp32_holds(v)]
    return bad


def scratch_image(t: np.ndarray) -> np.ndarray:
    """The 16x64 float image the liveness kernel leaves in scratch: slot
    r*64+lane is accumulator register r of lane `lane`, which holds
    D[(r&3) + 8*(r>>2) + 4*(lane>>5)][lane&31]."""
    img = np.empty((16, 64), dtype=np.float32)
    for r in range(16):
        for lane in range(64):
            img[r, lane] = t[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)][lane & 31]
    return img


def wrong_tile_models(nonce: int, iters: int) -> dict:
    """What plausible wrong kernels would produce instead of tile()."""
    a, b, c = tile_operands(nonce)
    t = c + iters * (a @ b)
    rows = np.arange(PROBE_M)
    return {
        "transposed_output": t.T.copy(),
        "ab_transposed": c + iters * (a @ b).T,
        "k_swapped_in_a": c + iters * (a[:, ::-1] @ b),
        "half_wave_rows_swapped": t[rows ^ 4].copy(),
        "iters_plus_1": c + (iters + 1) * (a @ b),
        "iters_minus_1": c + (iters - 1) * (a @ b),
        "only_k0": c + iters * np.outer(a[:, 0], b[0, :]),
        "c_dropped": iters * (a @ b),
    }


# ---- bf16 burn (mi355x_mfma_burn) ----------------------------------------------
def burn_operands(nonce: int):
    """A (32x16), B (16x32), C (32x16), D (16x32) as float64. Lane l holds, in
    element j of its fragments, A[l&31][8*(l>>5)+j] and B[8*(l>>5)+j][l&31];
    fragment x of a lane is burn_bf16_bits(l, j + 8*x), x = 0..3 for a, b, c, d."""
    mats = [np.zeros((32, 16)), np.zeros((16, 32)), np.zeros((32, 16)), np.zeros((16, 32))]
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for j in range(8):
            for x in range(4):
                v = bf16_value(burn_bf16_bits(lane, j + 8 * x, nonce))
                if x % 2 == 0:
                    mats[x][r, 8 * h + j] = v
                else:
                    mats[x][8 * h + j, r] = v
    return mats


def _burn_sums(a, b, c, d, iters):
    checksum = iters * float((a @ b).sum() - (c @ d).sum())
    abs_sum = iters * float((np.abs(a) @ np.abs(b)).sum() + (np.abs(c) @ np.abs(d)).sum())
    return checksum, abs_sum


def burn_checksum(nonce: int, iters: int):
    """(checksum, abs_sum) in float64: iters*(sum(A.B) - sum(C.D)) and
    iters*(sum(|A|.|B|) + sum(|C|.|D|))."""
    return _burn_sums(*burn_operands(nonce), iters)


def burn_bound(iters: int, abs_sum: float) -> float:
    """Any-order fp32 summation bound: every product passes through at most
    16*iters + 22 roundings (16 per MFMA over k, iters accumulations, 16
    registers, 6 cross-lane folds, with slack), each at most 2^-23 relative
    whether the unit truncates or rounds to nearest."""
    return (16 * iters + 22) * 2.0 ** -23 * abs_sum


BURN_MARGIN = 4      # for the MFMA's unspecified internal alignment


def wrong_burn_models(nonce: int, iters: int) -> dict:
    a, b, c, d = burn_operands(nonce)
    rev = np.r_[7:-1:-1, 15:7:-1]     # element j <-> 7-j within each lane's fragment
    swp = np.r_[8:16, 0:8]            # the two half-waves' k blocks exchanged
    return {
        "b_fragment_reversed": _burn_sums(a, b[rev, :], c, d[rev, :], iters)[0],
        "half_wave_k_blocks_swapped": _burn_sums(a[:, swp], b, c[:, swp], d, iters)[0],
        "iters_plus_1": _burn_sums(a, b, c, d, iters + 1)[0],
    }


# ---- comparisons on raw kernel outputs ------------------------------------------
def _bits(x) -> np.ndarray:
    return np.ascontiguousarray(x).view(np.uint32)


def assert_bit_equal(got, want, what: str) -> None:
    got, want = _bits(np.asarray(got)).ravel(), _bits(np.asarray(want)).ravel()
    assert got.shape == want.shape, f"{what}: {got.shape} words, want {want.shape}"
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (f"{what}: {diff.size}/{got.size} words differ, first at {int(diff[0])}: "
                            f"got {int(got[diff[0]]):#010x}, want {int(want[diff[0]]):#010x}")


def check_canaries(canaries: dict, fill: int) -> None:
    """Every guard byte before and after every buffer still holds `fill`."""
    assert canaries, "no canaries recorded"
    for name, arr in canaries.items():
        hit = np.flatnonzero(np.asarray(arr).ravel() != fill)
        assert hit.size == 0, f"{name}: {hit.size} guard bytes overwritten, first at offset {int(hit[0])}"


def check_liveness(out, scratch, meta, nonce: int, iters: int) -> None:
    want = tile_f32(nonce, iters)
    assert_bit_equal(out, want, "out")
    assert_bit_equal(scratch, scratch_image(want), "scratch")
    meta = np.asarray(meta, dtype=np.uint32)
    assert meta.shape == (4,)
    assert int(meta[META_MAGIC]) == PROBE_MAGIC, f"meta magic {int(meta[META_MAGIC]):#x}"
    assert int(meta[META_NONCE]) == nonce, f"meta nonce {int(meta[META_NONCE])}, want {nonce}"
    assert int(meta[META_XCC]) < NUM_XCC_MAX, f"meta xcc {int(meta[META_XCC])}"


SWEEP_WAVES = 4
ACC_REGS = 16


def accumulator_element(lane: int, reg: int) -> tuple:
    """(row, column) of the 32x32 tile that accumulator register `reg` of lane
    `lane` holds: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def sweep_wave_value(nonce: int, iters: int, wg: int, wave: int, lane: int, reg: int) -> int:
    """The exact integer in accumulator register `reg` of lane `lane` of that wave."""
    i, j = accumulator_element(lane, reg)
    return int(tile(sweep_nonce(nonce, wg, wave), iters)[i, j])


def sweep_injection_image(nonce: int, iters: int, grid: int, inject=None) -> dict:
    """What mi355x_chip_sweep of the test-only build must leave behind under
    `inject` (a raw_kernels request's "inject" object, or None for the hook
    off), from the documented layout alone: "mfma_bad" and "lds_bad" per
    workgroup, and "tiles" (grid, 32, 32) float32. A wrong word is counted once
    by the workgroup it is in and by no other; it reaches the host's tile only
    from wave 0, and there it differs from the healthy word by exactly the
    mask. An index outside the accumulator or the LDS pattern injects nothing."""
    mfma_bad, lds_bad = np.zeros(grid, dtype=np.int64), np.zeros(grid, dtype=np.int64)
    tiles = sweep_tiles(nonce, iters, grid).copy()
    if inject is not None and inject["mask"] & M32 and inject["wg"] < grid:
        wg, index, mask = inject["wg"], inject["index"], inject["mask"] & M32
        if inject["kind"] == "lds":
            if index < SWEEP_LDS_WORDS:
                lds_bad[wg] = 1
        else:
            assert inject["kind"] == "mfma", inject
            wave, lane = inject["wave"], inject["lane"]
            if wave < SWEEP_WAVES and lane < 64 and index < ACC_REGS:
                mfma_bad[wg] = 1
                if wave == 0:
                    i, j = accumulator_element(lane, index)
                    _bits(tiles)[wg, i, j] ^= np.uint32(mask)
    return {"mfma_bad": mfma_bad, "lds_bad": lds_bad, "tiles": tiles}


def check_sweep(records, tiles, nonce: int, iters: int, grid: int, inject=None) -> None:
    """`inject`: the injection the test-only build was asked for (sweep_injection_image)."""
    records = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)
    tiles = np.asarray(tiles, dtype=np.float32).reshape(grid, PROBE_M, PROBE_N)
    if inject is not None:
        want = sweep_injection_image(nonce, iters, grid, inject)
        for wg in range(grid):
            rec = [int(x) for x in records[wg]]
            assert rec[REC_MAGIC] == SWEEP_MAGIC and rec[REC_WG] == wg and rec[REC_NONCE] == nonce ^ wg, (wg, rec)
            assert rec[REC_MFMA_BAD] == want["mfma_bad"][wg], (
                f"wg {wg}: mfma_bad {rec[REC_MFMA_BAD]}, want {int(want['mfma_bad'][wg])} under {inject}")
            assert rec[REC_LDS_BAD] == want["lds_bad"][wg], (
                f"wg {wg}: lds_bad {rec[REC_LDS_BAD]}, want {int(want['lds_bad'][wg])} under {inject}")
            assert 1 <= rec[REC_ARRIVED] <= grid and rec[REC_XCC] < NUM_XCC_MAX, (wg, rec)
            assert_bit_equal(tiles[wg], want["tiles"][wg], f"wg {wg} tile under {inject}")
        return
    for wg in range(grid):
        rec = [int(x) for x in records[wg]]
        assert rec[REC_MAGIC] == SWEEP_MAGIC, f"wg {wg}: magic {rec[REC_MAGIC]:#x}"
        assert rec[REC_WG] == wg, f"wg {wg}: record says wg {rec[REC_WG]}"
        assert rec[REC_NONCE] == nonce ^ wg, f"wg {wg}: nonce word {rec[REC_NONCE]:#x}"
        assert rec[REC_MFMA_BAD] == 0, f"wg {wg}: mfma_bad {rec[REC_MFMA_BAD]}"
        assert rec[REC_LDS_BAD] == 0, f"wg {wg}: lds_bad {rec[REC_LDS_BAD]}"
        assert 1 <= rec[REC_ARRIVED] <= grid, f"wg {wg}: arrived {rec[REC_ARRIVED]}"
        t0 = rec[REC_T0_LO] | rec[REC_T0_HI] << 32
        t1 = rec[REC_T1_LO] | rec[REC_T1_HI] << 32
        assert t1 >= t0, f"wg {wg}: t1 {t1} < t0 {t0}"
        assert rec[REC_XCC] < NUM_XCC_MAX, f"wg {wg}: xcc {rec[REC_XCC]}"
        assert_bit_equal(tiles[wg], tile_f32(sweep_nonce(nonce, wg, 0), iters), f"wg {wg} tile")


def hbm_fill_image(n16: int, seed: int, poison_unit=None) -> np.ndarray:
    """What mi355x_hbm_fill must leave in the buffer (uint32 words)."""
    want = hbm_pattern_words(4 * n16, seed)
    if poison_unit is not None and poison_unit < n16:
        want[4 * poison_unit] ^= np.uint32(M32)
    return want


def check_hbm_fill(buf, n16: int, seed: int, poison_unit=None) -> None:
    assert_bit_equal(np.asarray(buf, dtype=np.uint32), hbm_fill_image(n16, seed, poison_unit), "buf")


def check_hbm_check(bad, first_bad, corrupt) -> None:
    """`corrupt`: the (unit, word) pairs the host corrupted. `bad` must count
    exactly those words and `first_bad` name the lowest such unit (all ones if none)."""
    words = {(int(u), int(w)) for u, w in corrupt}
    want_first = min((u for u, _ in words), default=M64)
    assert int(np.asarray(bad).ravel()[0]) == len(words), f"bad {int(np.asarray(bad).ravel()[0])}, want {len(words)}"
    got_first = int(np.asarray(first_bad).ravel()[0])
    assert got_first == want_first, f"first_bad {got_first:#x}, want {want_first:#x}"


def check_burn(records, counters_host, counters, nonce: int, iters: int, grid: int) -> float:
    """Asserts the burn records and returns |gpu - ref| / bound of the checksum."""
    records = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)
    for wg in range(grid):
        rec = [int(x) for x in records[wg]]
        assert rec[PREC_MAGIC] == PERF_MAGIC, f"wg {wg}: magic {rec[PREC_MAGIC]:#x}"
        assert rec[PREC_WG] == wg, f"wg {wg}: record says wg {rec[PREC_WG]}"
        assert rec[PREC_NONCE] == nonce ^ wg, f"wg {wg}: nonce word {rec[PREC_NONCE]:#x}"
        rt0 = rec[PREC_RT0_LO] | rec[PREC_RT0_HI] << 32
        rt1 = rec[PREC_RT1_LO] | rec[PREC_RT1_HI] << 32
        assert rt1 >= rt0, f"wg {wg}: rt1 {rt1} < rt0 {rt0}"
        assert rec[PREC_CYC_LO] | rec[PREC_CYC_HI] << 32 > 0, f"wg {wg}: no shader clock ticks"
        assert rec[PREC_XCC] < NUM_XCC_MAX, f"wg {wg}: xcc {rec[PREC_XCC]}"
    assert_bit_equal(np.asarray(counters_host, dtype=np.uint32), np.asarray(counters, dtype=np.uint32),
                     "hbm_counters_host")
    sums = np.ascontiguousarray(records[:, PREC_SUM:PREC_SUM + 4]).ravel()
    assert (sums == sums[0]).all(), f"checksums differ between waves: {[hex(int(s)) for s in sums]}"
    ratio = burn_ratio(records, nonce, iters)
    assert ratio <= BURN_MARGIN, (f"checksum {burn_gpu_checksum(records)!r} vs reference "
                                  f"{burn_checksum(nonce, iters)[0]!r}: |diff| is {ratio:.3f} x bound, "
                                  f"allowed {BURN_MARGIN}")   # a NaN ratio fails too
    return ratio


def burn_gpu_checksum(records) -> float:
    """Workgroup 0 wave 0's checksum word as a float."""
    words = np.asarray(records, dtype=np.uint32).ravel()[PREC_SUM:PREC_SUM + 1].copy()
    return float(words.view(np.float32)[0])


def burn_ratio(records, nonce: int, iters: int) -> float:
    """|gpu - ref| / bound for the checksum in `records`."""
    ref, abs_sum = burn_checksum(nonce, iters)
    return abs(burn_gpu_checksum(records) - ref) / burn_bound(iters, abs_sum)


# ---- what the host decides from the records (chip_verify.h) --------------------
# Written from the field comments of mi355x_sweep_result / mi355x_perf_result
# (liveness_probe.h) and the record words above, in Python ints: the keys are
# the keys of the probe's JSON object, for the fields the records and the
# caller's inputs determine (the rest -- ordinal, dispatch times -- belong to the
# dispatch, not the verdict).
SWEEP_FLOAT_DIGITS = {"arrival_spread_us": 2}
PERF_FLOAT_DIGITS = {"fill_us": 1, "check_us": 1, "check2_us": 1, "mfma_us": 1, "hbm_write_gbps": 1,
                     "hbm_read_gbps": 1, "mfma_tflops": 1, "clock_mhz_min": 0, "clock_mhz_median": 0,
                     "clock_mhz_max": 0, "xcd_clock_mhz": 0}
BURN_WAVES = 4
MFMA_FLOPS = 2 * 32 * 32 * 16          # one v_mfma_f32_32x32x16
REALTIME_MHZ = 100                     # s_memrealtime
COUNTER_FILL_WORD = 0xA5A5A5A5         # the host counter words before the burn kernel's copy

_sweep_tiles_cache: dict = {}


def sweep_tiles(nonce: int, iters: int, grid: int) -> np.ndarray:
    """Wave 0's tile of every workgroup, float32 (grid, 32, 32). Computed once
    per (nonce, iters, grid) and read-only: copy before changing it."""
    key = (nonce, iters, grid)
    if key not in _sweep_tiles_cache:
        t = np.stack([tile_f32(sweep_nonce(nonce, wg, 0), iters) for wg in range(grid)])
        t.setflags(write=False)
        _sweep_tiles_cache[key] = t
    return _sweep_tiles_cache[key]


def spread_placement(grid: int, xcds: int) -> list:
    """(xcc, cu-bits) per workgroup: workgroups dealt round-robin to the XCDs,
    each to the next CU of its XCD."""
    return [(wg % xcds, wg // xcds) for wg in range(grid)]


def healthy_sweep(grid: int, nonce: int, iters: int, placement):
    """(records, tiles) a correct mi355x_chip_sweep would write: every
    workgroup saw the whole grid, arrivals one tick apart."""
    placement = list(placement)
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        t0 = 0x12_0000_0000 + wg
        t1 = t0 + 5000
        recs[wg, REC_MAGIC], recs[wg, REC_NONCE], recs[wg, REC_WG] = SWEEP_MAGIC, nonce ^ wg, wg
        recs[wg, REC_XCC], recs[wg, REC_HWID], recs[wg, REC_ARRIVED] = xcc, (cu << 8) | 0x3, grid
        recs[wg, REC_T0_LO], recs[wg, REC_T0_HI] = t0 & M32, t0 >> 32
        recs[wg, REC_T1_LO], recs[wg, REC_T1_HI] = t1 & M32, t1 >> 32
    return recs, sweep_tiles(nonce, iters, grid).copy()


def _per_wg(value, grid: int) -> list:
    return [int(value)] * grid if np.isscalar(value) else [int(v) for v in value]


def healthy_burn(burn_wgs: int, nonce: int, placement, cyc, rt_ticks, checksum_word: int) -> np.ndarray:
    """The records a correct mi355x_mfma_burn would write; `cyc` (shader clock
    ticks) and `rt_ticks` (100 MHz ticks) over the loop, one value or one per
    workgroup; every wave's checksum is `checksum_word`."""
    placement = list(placement)
    assert len(placement) == burn_wgs
    cyc, rt_ticks = _per_wg(cyc, burn_wgs), _per_wg(rt_ticks, burn_wgs)
    recs = np.zeros((burn_wgs, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        rt0 = 0xFFFF_FF00 + 7 * wg                       # some intervals straddle 2^32
        rt1 = rt0 + rt_ticks[wg]
        recs[wg, PREC_MAGIC], recs[wg, PREC_WG], recs[wg, PREC_NONCE] = PERF_MAGIC, wg, nonce ^ wg
        recs[wg, PREC_XCC], recs[wg, PREC_HWID] = xcc, (cu << 8) | 0x1
        recs[wg, PREC_RT0_LO], recs[wg, PREC_RT0_HI] = rt0 & M32, rt0 >> 32
        recs[wg, PREC_RT1_LO], recs[wg, PREC_RT1_HI] = rt1 & M32, rt1 >> 32
        recs[wg, PREC_CYC_LO], recs[wg, PREC_CYC_HI] = cyc[wg] & M32, cyc[wg] >> 32
        recs[wg, PREC_SUM:PREC_SUM + BURN_WAVES] = checksum_word
    return recs


def _xcd_entries(num_xcc: int) -> int:
    """How many per-XCD entries the JSON carries: the agent's XCDs, 8 when it named none."""
    return min(16, num_xcc if num_xcc > 0 else NUM_XCC_MAX)


def _median(values) -> float:
    return sorted(values)[len(values) // 2] if values else 0.0


# The verdict judges records; which agent wrote them is the caller's to say
# (hsa_chip.cpp fills kfd_node_id and pci_bus_id once it has reached the
# device). A verdict on records alone carries "no agent".
NO_AGENT = {"kfd_node_id": -1, "pci_bus_id": ""}


def sweep_verdict(records, tiles, grid: int, nonce: int, iters: int, num_xcc: int) -> dict:
    rec = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS).astype(np.uint64)
    got = _bits(np.asarray(tiles, dtype=np.float32)).reshape(grid, PROBE_M * PROBE_N)
    want = _bits(sweep_tiles(nonce, iters, grid)).reshape(grid, PROBE_M * PROBE_N)
    wrong = (got != want).sum(axis=1)
    wgs = np.arange(grid, dtype=np.uint64)
    present = ((rec[:, REC_MAGIC] == SWEEP_MAGIC) & (rec[:, REC_WG] == wgs)
               & (rec[:, REC_NONCE] == (np.uint64(nonce) ^ wgs)))
    good = present & (rec[:, REC_MFMA_BAD] == 0) & (rec[:, REC_LDS_BAD] == 0) & (wrong == 0)
    seen = rec[present]                                    # absent records count for nothing
    xccs = [int(x) & 0xF for x in seen[:, REC_XCC]]
    cus = [int(h) >> 8 & 0xFF for h in seen[:, REC_HWID]]
    arrivals = [int(lo) | int(hi) << 32 for lo, hi in zip(seen[:, REC_T0_LO], seen[:, REC_T0_HI])]
    records_ok = int(good.sum())
    out = {
        "nonce": nonce, "iters": iters, "grid": grid, "num_xcc": num_xcc,
        "records_ok": records_ok,
        "mfma_bad": sum(int(x) for x in seen[:, REC_MFMA_BAD]) & M32,      # a uint32_t field
        "lds_bad": sum(int(x) for x in seen[:, REC_LDS_BAD]) & M32,
        "tile_bad": int(wrong[present].sum()),
        "cus_covered": len(set(zip(xccs, cus))),
        "xccs_covered": len(set(xccs)),
        "all_resident": records_ok == grid and all(int(a) >= grid for a in seen[:, REC_ARRIVED]),
        "wgs_per_xcc": [xccs.count(x) for x in range(_xcd_entries(num_xcc))],
        "arrival_spread_us": (max(arrivals) - min(arrivals)) / REALTIME_MHZ if arrivals else 0.0,
    }
    out["ok"] = records_ok == grid and (num_xcc <= 0 or out["xccs_covered"] == num_xcc)
    out.update(NO_AGENT)
    return out


def _finite_f32_word(word: int) -> bool:
    return word >> 23 & 0xFF != 0xFF


def perf_verdict(records, counters, burn_wgs: int, nonce: int, num_xcc: int, bytes: int, mfma_iters: int,  # noqa: A002
                 fill_us: float, check_us: float, check2_us: float, mfma_us: float) -> dict:
    recs = [[int(x) for x in row] for row in np.asarray(records, dtype=np.uint32).reshape(burn_wgs, REC_WORDS)]
    pass1, pass2, first_lo, first_hi = (int(x) for x in np.asarray(counters, dtype=np.uint32).ravel())
    first = first_lo | first_hi << 32
    present = [wg for wg, r in enumerate(recs)
               if r[PREC_MAGIC] == PERF_MAGIC and r[PREC_WG] == wg and r[PREC_NONCE] == nonce ^ wg]
    sums = [recs[wg][PREC_SUM + v] for wg in present for v in range(BURN_WAVES)]
    if sums and _finite_f32_word(sums[0]):
        mismatch = sum(1 for s in sums if s != sums[0])
    else:
        mismatch = len(sums)              # a NaN / Inf checksum agrees with nothing, itself included
    clocks, per_xcd = [], [[] for _ in range(16)]
    for wg in present:
        r = recs[wg]
        ticks = (r[PREC_RT1_LO] | r[PREC_RT1_HI] << 32) - (r[PREC_RT0_LO] | r[PREC_RT0_HI] << 32)
        if ticks > 0:
            mhz = (r[PREC_CYC_LO] | r[PREC_CYC_HI] << 32) / (ticks / REALTIME_MHZ)
            clocks.append(mhz)
            per_xcd[r[PREC_XCC] & 0xF].append(mhz)
    reads = [t for t in (check_us, check2_us) if t > 0]
    flops = MFMA_FLOPS * 2 * mfma_iters * BURN_WAVES * burn_wgs
    xccs = {recs[wg][PREC_XCC] & 0xF for wg in present}
    out = {
        "nonce": nonce, "bytes": bytes, "num_xcc": num_xcc, "mfma_iters": mfma_iters, "mfma_grid": burn_wgs,
        "fill_us": fill_us, "check_us": check_us, "check2_us": check2_us, "mfma_us": mfma_us,
        "hbm_write_gbps": bytes / (fill_us * 1e3) if fill_us > 0 else 0.0,
        "hbm_read_gbps": bytes / (min(reads) * 1e3) if reads else 0.0,
        "hbm_bad_words": max(pass1, pass2), "hbm_bad_words_pass2": pass2,
        "hbm_first_bad": first if first < bytes // 16 else -1,
        "mfma_records_ok": len(present), "mfma_checksum_mismatch": mismatch, "mfma_xccs": len(xccs),
        "mfma_tflops": flops / (mfma_us * 1e6) if mfma_us > 0 else 0.0,
        "clock_mhz_min": min(clocks, default=0.0), "clock_mhz_median": _median(clocks),
        "clock_mhz_max": max(clocks, default=0.0),
        "xcd_clock_mhz": [_median(c) for c in per_xcd][:_xcd_entries(num_xcc)],
    }
    out["ok"] = (out["hbm_bad_words"] == 0 and mismatch == 0 and len(present) == burn_wgs
                 and (num_xcc <= 0 or len(xccs) == num_xcc))
    out.update(NO_AGENT)
    return out


def float_tolerance(want: float, digits: int) -> float:
    """What a value printed with `digits` decimals may differ by after parsing:
    half a unit of the last digit, plus 1e-9 relative for the few double
    operations whose order may differ."""
    return 0.5 * 10.0 ** -digits + 1e-9 * abs(want)


def assert_verdict(got: dict, want: dict, float_digits: dict, what: str = "") -> None:
    """`got`: a parsed JSON line of the probe; `want`: sweep_verdict / perf_verdict.
    Integers and booleans equal exactly, printed doubles within float_tolerance."""
    for key, w in want.items():
        assert key in got, f"{what}: no {key!r} in {sorted(got)}"
        g = got[key]
        if key in float_digits:
            gs, ws = (g, w) if isinstance(w, list) else ([g], [w])
            assert len(gs) == len(ws), f"{what}: {key} {g} want {w}"
            for a, b in zip(gs, ws):
                assert abs(a - b) <= float_tolerance(b, float_digits[key]), f"{what}: {key} {g} want {w}"
        else:
            assert type(g) is type(w) and g == w, f"{what}: {key} {g!r} want {w!r}"
