"""Independent reference for the bf16 MFMA datapath check
(mi355x_mfma_datapath_bf16, native/src/health/datapath_bf16_kernel.h,
datapath_bf16_verify.h).

Written from the recipe in the header's comment, in Python integers: a number
is a pair (m, e) standing for m * 2^e, a product multiplies the m and adds the
e, a sum aligns to the smallest e. Nothing here rounds: `f32_word` refuses a
value that is not exactly an f32, and `terms` / `quantum` hand the tests what
they need to show that no partial sum, in any order, can need more than 24
bits.

Also: the record / tile image a correct kernel writes, the verdict the host
draws from them, wrong-kernel and stuck-bit models (those do round, to nearest
even, since a wrong kernel's sums need not be exact), and a driver for
native/tests/datapath_bf16_contract_cli.cpp.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
CLI_SOURCE = REPO / "native" / "tests" / "datapath_bf16_contract_cli.cpp"
CLI_INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

M32 = 0xFFFFFFFF
STAGES = 5
DIM = (32, 32, 32, 32, 16)          # rows = columns of a stage's tile
BLOCKS = (2, 2, 2, 2, 4)            # K-blocks of a stage's instruction; a block is 4 dwords = 8 bf16
DWORDS = 4
DEPTH = tuple(8 * b for b in BLOCKS)  # K
TILE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = (0, 1024, 2048, 3072, 4096)
WG_WORDS = 4 * 1024 + 256
REC_WORDS = 16
WAVES = 4
THREADS = 256
MAGIC = int.from_bytes(b"DPBF", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8

GOLDEN, MURMUR = 0x9E3779B1, 0x85EBCA77
SEL_A, SEL_B, SEL_C, SEL_SIGN, SEL_ROT, SEL_EA, SEL_EB = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800, 0x3900, 0x3A00
BAND = range(97, 159)               # exponent fields of a bf16 band word
C_BAND = range(1, 255)              # exponent fields of stage 3's C
ONE_HOT_A, ONE_HOT_B = (1,), (0,)   # the stages whose A / B operand is one-hot
ZERO_A = (3,)
PRODUCT_STAGES = (2, 4)
F_RANGE = range(-90, 91)            # the one-hot entries are +-2^f


# ---- integer hashes ---------------------------------------------------------------
def wave_nonce(nonce: int, wg: int, wave: int) -> int:
    return ((nonce ^ wg * GOLDEN & M32) + wave * MURMUR) & M32


def mix(nw: int, stage: int, selector: int) -> int:
    h = nw ^ ((stage + 0x21) * GOLDEN & M32) ^ (selector * MURMUR & M32)
    for shift, mult in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h ^= h >> shift
        h = h * mult & M32
    return h ^ h >> 16


# ---- numbers: (m, e) is m * 2^e --------------------------------------------------
def bf16_value(h: int) -> tuple:
    sign, e, m = h >> 15, h >> 7 & 0xFF, h & 0x7F
    assert e != 255, hex(h)
    mag, exp = (m, -133) if e == 0 else (128 + m, e - 134)
    return (-mag if sign else mag, exp)


def f16_value(h: int) -> tuple:
    """The same 16 bits read as IEEE half (a wrong-kernel model)."""
    sign, e, m = h >> 15, h >> 10 & 0x1F, h & 0x3FF
    assert e != 31, hex(h)
    mag, exp = (m, -24) if e == 0 else (1024 + m, e - 25)
    return (-mag if sign else mag, exp)


def f32_value(w: int) -> tuple:
    sign, e, m = w >> 31, w >> 23 & 0xFF, w & 0x7FFFFF
    assert e != 255, hex(w)
    mag, exp = (m, -149) if e == 0 else ((1 << 23) + m, e - 150)
    return (-mag if sign else mag, exp)


def total(terms) -> tuple:
    lo = min(e for _, e in terms)
    return (sum(m << (e - lo) for m, e in terms), lo)


def f32_round(value: tuple) -> int:
    """The f32 word nearest to m * 2^e, ties to even (+0 for zero)."""
    m, e = value
    if m == 0:
        return 0
    sign, a = (0x80000000 if m < 0 else 0), abs(m)
    biased = a.bit_length() - 1 + e + 127
    q = -149 if biased <= 0 else a.bit_length() - 1 + e - 23     # exponent of the result's last place
    shift = q - e
    if shift <= 0:
        sig = a << -shift
    else:
        sig, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        sig += rem > half or (rem == half and sig & 1)
    word = sig if biased <= 0 else ((biased - 1) << 23) + sig    # a carry out of the significand moves the exponent
    return sign | min(word, 0x7F800000)


def f32_word(value: tuple) -> int:
    """The f32 word that is exactly m * 2^e; a value that is no normal f32 is an error."""
    w = f32_round(value)
    got, (m, e) = f32_value(w), value
    lo = min(e, got[1])
    assert m << (e - lo) == got[0] << (got[1] - lo) and 1 <= (w >> 23 & 0xFF) <= 254, (value, hex(w))
    return w


def halves(word: int) -> tuple:
    """The two 16-bit elements of a fragment dword, the even element first."""
    return word & 0xFFFF, word >> 16


# ---- operand words ------------------------------------------------------------------
def band16(h16: int) -> int:
    return (h16 & 0x807F) | (BAND[0] + ((h16 >> 7 & 0xFF) * len(BAND) >> 8)) << 7


def _band(nw: int, stage: int, selector: int, rc: int, block: int, dword: int) -> int:
    """Band words; dword 1 is the complement of dword 0, dword 3 of dword 2."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 4 + dword // 2 * 2)
    w = band16(h & 0xFFFF) | band16(h >> 16) << 16
    return w ^ M32 if dword % 2 else w


def onehot_position(stage: int, rc: int, nw: int) -> int:
    """The k (0..15) where row / column `rc` of a one-hot operand is not zero."""
    return (rc + mix(nw, stage, SEL_ROT) % 16) % 16


def onehot_entry(stage: int, rc: int, nw: int) -> int:
    """The bf16 pattern of +-2^f there."""
    h = mix(nw, stage, SEL_SIGN + rc)
    return (h >> 31) << 15 | (127 + F_RANGE[0] + (h & 0xFFFF) % len(F_RANGE)) << 7


def _onehot(nw: int, stage: int, rc: int, block: int, dword: int) -> int:
    pos = onehot_position(stage, rc, nw)
    if pos // 2 != block * DWORDS + dword:
        return 0
    return onehot_entry(stage, rc, nw) << 16 * (pos % 2)


def exponent_field(nw: int, stage: int, selector: int, rc: int) -> int:
    return BAND[0] + mix(nw, stage, selector + rc) % len(BAND)


def _odd(nw: int, stage: int, selector: int, rc: int, block: int, dword: int, e: int) -> int:
    """Two elements +-(128 + m) * 2^(e - 134), m odd."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 4 + dword)
    return (h & 0x807F807F) | 0x00010001 | e << 7 | e << 23


def a_word(stage: int, row: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_A:
        return _onehot(nw, stage, row, block, dword)
    if stage in ZERO_A:
        return 0
    if stage in PRODUCT_STAGES:
        return _odd(nw, stage, SEL_A, row, block, dword, exponent_field(nw, stage, SEL_EA, row))
    return _band(nw, stage, SEL_A, row, block, dword)


def b_word(stage: int, col: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_B:
        return _onehot(nw, stage, col, block, dword)
    if stage in PRODUCT_STAGES:
        return _odd(nw, stage, SEL_B, col, block, dword, exponent_field(nw, stage, SEL_EB, col))
    return _band(nw, stage, SEL_B, col, block, dword)


def quantum(stage: int, row: int, col: int, nw: int) -> int:
    """Stages 2 and 4: the exponent x of q = 2^x, of which C and every product of D[row][col] are multiples."""
    return exponent_field(nw, stage, SEL_EA, row) + exponent_field(nw, stage, SEL_EB, col) - 268


def c_word(stage: int, row: int, col: int, nw: int) -> int:
    if stage in PRODUCT_STAGES:
        h = mix(nw, stage, SEL_C + 32 * row + col)
        ga = (h & 0xFFFFF) | 1
        return f32_word((-ga if h >> 31 else ga, quantum(stage, row, col, nw)))
    if stage == 3:
        h = mix(nw, 3, SEL_C + 32 * row + (0 if col == 1 else col))
        w = (h & 0x807FFFFF) | (C_BAND[0] + ((h >> 23 & 0xFF) * len(C_BAND) >> 8)) << 23
        return w ^ M32 if col == 1 else w
    return 0


@lru_cache(maxsize=None)
def operands(stage: int, nw: int):
    """(A words [dim][blocks*4], B words [dim][blocks*4], C words [dim][dim]) of one
    wave's stage; operand word block*4 + dword of a row / column holds k = 2 * word and 2 * word + 1."""
    dim, words = DIM[stage], BLOCKS[stage] * DWORDS
    a = tuple(tuple(a_word(stage, i, w // 4, w % 4, nw) for w in range(words)) for i in range(dim))
    b = tuple(tuple(b_word(stage, j, w // 4, w % 4, nw) for w in range(words)) for j in range(dim))
    c = tuple(tuple(c_word(stage, i, j, nw) for j in range(dim)) for i in range(dim))
    return a, b, c


def elements(fragment) -> list:
    """The 16-bit patterns of a row / column in k order."""
    return [h for word in fragment for h in halves(word)]


def _values(fragment, decode=bf16_value) -> list:
    return [decode(h) for h in elements(fragment)]


def terms(stage: int, nw: int, row: int, col: int) -> list:
    """C and the K products of D[row][col], each as (m, e)."""
    a, b, c = operands(stage, nw)
    return [f32_value(c[row][col])] + [(x * y, ex + ey) for (x, ex), (y, ey) in zip(_values(a[row]), _values(b[col]))]


@lru_cache(maxsize=None)
def expected_tile(stage: int, nw: int) -> tuple:
    """The output words of one wave's stage, row-major: C + sum over k of A * B, exactly."""
    a, b, c = operands(stage, nw)
    av, bv = [_values(f) for f in a], [_values(f) for f in b]
    dim = DIM[stage]
    out = []
    for i in range(dim):
        for j in range(dim):
            parts = [f32_value(c[i][j])] + [(x * y, ex + ey) for (x, ex), (y, ey) in zip(av[i], bv[j])]
            out.append(f32_word(total(parts)))
    return tuple(out)


def _both(words) -> int:
    ones = zeros = 0
    for w in words:
        ones, zeros = ones | w, zeros | (w ^ M32)
    return ones & zeros


def toggle_masks(nw: int) -> dict:
    """Per operand, the bits that take both values: in every single fragment
    (the four dwords one lane hands the instruction) of A in stage 0 and of B
    in stage 1, in every row of C in stage 3, and in every row of D in stage 3."""
    a0, _, _ = operands(0, nw)
    _, b1, _ = operands(1, nw)
    _, _, c3 = operands(3, nw)
    d3 = expected_tile(3, nw)

    def every(groups) -> int:
        out = M32
        for g in groups:
            out &= _both(g)
        return out

    def fragments(rows) -> list:
        return [row[4 * h:4 * h + 4] for row in rows for h in range(len(row) // 4)]
    return {"A": every(fragments(a0)), "B": every(fragments(b1)), "C": every(c3),
            "D": every(d3[32 * i:32 * i + 32] for i in range(32))}


def selected_positions(stage: int, nw: int) -> list:
    """Stage 0 / 1: per column / row, the k its one-hot entry selects, read back
    from the operand words (not from onehot_position)."""
    a, b, _ = operands(stage, nw)
    frags = b if stage in ONE_HOT_B else a
    out = []
    for f in frags:
        nz = [k for k, h in enumerate(elements(f)) if h]
        assert len(nz) == 1, (stage, f)
        out.append(nz[0])
    return out


# ---- what a correct kernel writes ----------------------------------------------------
_tiles_cache: dict = {}


def tiles_image(nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][4352] as uint32: wave 0's five tiles of every workgroup, four
    of 32x32 and one of 16x16. Computed once per (nonce, grid) and read-only:
    copy before changing it."""
    key = (nonce, grid)
    if key not in _tiles_cache:
        t = np.array([[w for s in range(STAGES) for w in expected_tile(s, wave_nonce(nonce, wg, 0))]
                      for wg in range(grid)], dtype=np.uint32).reshape(grid, WG_WORDS)
        t.setflags(write=False)
        _tiles_cache[key] = t
    return _tiles_cache[key]


def spread_placement(grid: int, xcds: int = 8) -> list:
    """(xcc, cu-bits) per workgroup: dealt round-robin to the XCDs."""
    return [(wg % xcds, wg // xcds) for wg in range(grid)]


def healthy(grid: int, nonce: int, placement=None):
    """(records, tiles) a correct mi355x_mfma_datapath_bf16 would write; wave v of
    a workgroup on SIMD v of its CU."""
    placement = list(placement or spread_placement(grid))
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        recs[wg, REC_MAGIC], recs[wg, REC_WG], recs[wg, REC_NONCE], recs[wg, REC_XCC] = MAGIC, wg, nonce ^ wg, xcc
        for v in range(WAVES):
            recs[wg, REC_HWID + v] = cu << 8 | v << 4 | 0x1
    return recs, tiles_image(nonce, grid).copy()


ACC_REGS = (16, 16, 16, 16, 4)
INDEX_STRIDE = 16                   # inject index = stage * 16 + register


def accumulator_element(stage: int, lane: int, reg: int) -> tuple:
    """(row, column) of the stage's tile that accumulator register `reg` of lane
    `lane` holds: 32x32: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]; 16x16: D[4*(l>>4) + r][l&15]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS[stage]
    if DIM[stage] == 16:
        return 4 * (lane >> 4) + reg, lane & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def injection_image(nonce: int, grid: int, inject=None) -> tuple:
    """(stage_bad (grid, 5), tiles (grid, 4352) uint32) that
    mi355x_mfma_datapath_bf16 of the test-only build must leave behind under
    `inject` (a raw_kernels request's "inject" object: index = stage * 16 +
    register; None for the hook off), from the documented layout alone. The
    wrong word is counted once, by its workgroup, in its stage's counter; it
    reaches the host's tiles only from wave 0, and there it differs from the
    healthy word by exactly the mask. An index that names no register injects nothing."""
    stage_bad = np.zeros((grid, STAGES), dtype=np.int64)
    tiles = tiles_image(nonce, grid).copy()
    if inject is not None and inject["mask"] & M32 and inject["wg"] < grid:
        assert inject["kind"] == "mfma", inject
        wg, wave, lane, index = inject["wg"], inject["wave"], inject["lane"], inject["index"]
        stage, reg = divmod(index, INDEX_STRIDE)
        if wave < WAVES and lane < 64 and stage < STAGES and reg < ACC_REGS[stage]:
            stage_bad[wg, stage] = 1
            if wave == 0:
                i, j = accumulator_element(stage, lane, reg)
                tiles[wg, TILE_OFFSET[stage] + i * DIM[stage] + j] ^= np.uint32(inject["mask"] & M32)
    return stage_bad, tiles


HW_WORDS = (REC_XCC, REC_HWID, REC_HWID + 1, REC_HWID + 2, REC_HWID + 3)   # hardware's, not the reference's


def check_raw(records, tiles, nonce: int, grid: int, inject=None) -> None:
    """Every word the kernel wrote against the reference image: the whole tile
    buffer, and the records but for where the workgroup ran (those: XCC id in
    range, HW_ID words non-zero). `inject`: the injection the test-only build
    was asked for (injection_image)."""
    rec = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)
    til = np.asarray(tiles, dtype=np.uint32).reshape(grid, WG_WORDS)
    want_rec, _ = healthy(grid, nonce)
    want_bad, want_tiles = injection_image(nonce, grid, inject)
    want_rec[:, REC_BAD:REC_BAD + STAGES] = want_bad
    bad = np.argwhere(til != want_tiles)
    if bad.size:
        wg, w = (int(x) for x in bad[0])
        stage = max(s for s in range(STAGES) if TILE_OFFSET[s] <= w)
        per_stage = [int(((bad[:, 1] >= TILE_OFFSET[s]) & (bad[:, 1] < TILE_OFFSET[s] + TILE_WORDS[s])).sum())
                     for s in range(STAGES)]
        raise AssertionError(f"nonce {nonce:#x} grid {grid}: {len(bad)} tile words differ (per stage {per_stage}), "
                             f"first wg {wg} stage {stage} word {w - TILE_OFFSET[stage]}: got {int(til[wg, w]):#010x} "
                             f"want {int(want_tiles[wg, w]):#010x}")
    keep = [w for w in range(REC_WORDS) if w not in HW_WORDS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, inject, rec[:, keep].tolist())
    assert (rec[:, REC_BAD:REC_BAD + STAGES] == want_bad).all(), (inject, rec[:, REC_BAD:REC_BAD + STAGES].tolist())
    assert (rec[:, REC_XCC] < 16).all(), rec[:, REC_XCC].tolist()
    assert (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec[:, REC_HWID:REC_HWID + WAVES].tolist()


# ---- fault and wrong-kernel models (on the tile image) ------------------------------
def stuck_bit(tiles: np.ndarray, bit: int, value: int) -> np.ndarray:
    t = np.array(tiles, dtype=np.uint32)
    return t | np.uint32(1 << bit) if value else t & np.uint32(~(1 << bit) & M32)


def _stuck_words(words, bit: int, value: int) -> list:
    return [w | 1 << bit if value else w & ~(1 << bit) & M32 for w in words]


def _blocks_swapped(words) -> list:
    blocks = [words[k:k + 4] for k in range(0, len(words), 4)]
    return [w for blk in blocks[1:] + blocks[:1] for w in blk]


def _elements_reversed(words) -> list:
    """Element e of each fragment (four dwords) where element 7 - e belongs."""
    out = []
    for k in range(0, len(words), 4):
        el = elements(words[k:k + 4])[::-1]
        out += [el[2 * d] | el[2 * d + 1] << 16 for d in range(4)]
    return out


def _top8(product: tuple) -> tuple:
    m, e = product
    drop = max(abs(m).bit_length() - 8, 0)
    return ((abs(m) >> drop << drop) * (-1 if m < 0 else 1), e)


def _model(nw: int, stage: int, fix_a=None, fix_b=None, fix_c=None, decode=bf16_value, fix_product=None) -> list:
    """A stage's tile with a change applied to A's words, B's words, C's word,
    the decoding or each product; rounded to nearest even where it is not exact."""
    a, b, c = operands(stage, nw)
    dim = DIM[stage]
    av = [_values(fix_a(list(f)) if fix_a else f, decode) for f in a]
    bv = [_values(fix_b(list(f)) if fix_b else f, decode) for f in b]
    out = []
    for i in range(dim):
        for j in range(dim):
            cw = fix_c(c[i][j]) if fix_c else c[i][j]
            if cw is not None and cw >> 23 & 0xFF == 255:
                out.append(cw)                      # an Inf or NaN in C comes out as it went in
                continue
            prods = [(x * y, ex + ey) for (x, ex), (y, ey) in zip(av[i], bv[j])]
            if fix_product:
                prods = [fix_product(p) for p in prods]
            out.append(f32_round(total(([f32_value(cw)] if cw is not None else []) + prods)))
    return out


STUCK_MODELS = {"A bit 20 stuck at 0": ("a", 20, 0), "B bit 5 stuck at 1": ("b", 5, 1), "C bit 12 stuck at 1": ("c", 12, 1),
                "D bit 30 stuck at 0": ("d", 30, 0)}


def wrong_kernel_models(nonce: int, grid: int) -> dict:
    """Tile images of kernels (or of a unit) that get the instruction's contract wrong."""
    good = tiles_image(nonce, grid)

    def rebuilt(**how):
        return np.array([[w for s in range(STAGES) for w in _model(wave_nonce(nonce, wg, 0), s, **how)]
                         for wg in range(grid)], dtype=np.uint32).reshape(good.shape)

    out = {
        "fragment element order of A reversed": rebuilt(fix_a=_elements_reversed),
        "A's K-blocks of the lane halves swapped": rebuilt(fix_a=_blocks_swapped),
        "operands decoded as f16": rebuilt(decode=f16_value),
        "products truncated to their top 8 bits": rebuilt(fix_product=_top8),
        "C dropped": rebuilt(fix_c=lambda w: None),
    }
    for name, (what, bit, value) in STUCK_MODELS.items():
        if what == "d":
            out[name] = stuck_bit(good, bit, value)
        elif what == "c":
            out[name] = rebuilt(fix_c=lambda w: _stuck_words([w], bit, value)[0])
        else:
            out[name] = rebuilt(**{"fix_" + what: lambda ws: _stuck_words(ws, bit, value)})
    return out


# ---- the verdict (datapath_bf16_verify.h), from the field comments of mi355x_datapath_bf16_result ----
def verdict(records, tiles, grid: int, nonce: int) -> dict:
    rec = [[int(x) for x in row] for row in np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)]
    got = np.asarray(tiles, dtype=np.uint32).reshape(grid, WG_WORDS)
    want = tiles_image(nonce, grid)
    present = [wg for wg, r in enumerate(rec)
               if r[REC_MAGIC] == MAGIC and r[REC_WG] == wg and r[REC_NONCE] == nonce ^ wg]
    stage_bad = [sum(rec[wg][REC_BAD + s] for wg in present) & M32 for s in range(STAGES)]
    wrong = {wg: np.flatnonzero(got[wg] != want[wg]) for wg in present}
    first = next(((wg, int(w[0])) for wg, w in wrong.items() if w.size), None)
    xccs = [rec[wg][REC_XCC] & 0xF for wg in present]
    cus = {(rec[wg][REC_XCC] & 0xF, rec[wg][REC_HWID] >> 8 & 0xFF) for wg in present}
    simds = {(rec[wg][REC_XCC] & 0xF, rec[wg][REC_HWID + v] >> 8 & 0xFF, rec[wg][REC_HWID + v] >> 4 & 0x3)
             for wg in present for v in range(WAVES)}
    records_ok = sum(1 for wg in present if not wrong[wg].size and not any(rec[wg][REC_BAD:REC_BAD + STAGES]))
    out = {
        "nonce": nonce, "grid": grid, "records_ok": records_ok,
        "mfma_bad": sum(sum(rec[wg][REC_BAD:REC_BAD + STAGES]) for wg in present) & M32,
        "stage_bad": stage_bad,
        "tile_bad": sum(int(w.size) for w in wrong.values()),
        "first_bad_wg": -1, "first_bad_stage": -1, "first_bad_word": -1,
        "first_bad_got": 0, "first_bad_want": 0, "first_bad_xor": 0,
        "cus_covered": len(cus), "simds_covered": len(simds), "xccs_covered": len(set(xccs)),
        "ok": records_ok == grid,
        "kfd_node_id": -1, "pci_bus_id": "",        # a verdict on records alone names no agent (hsa_chip.cpp does)
    }
    if first:
        wg, w = first
        stage = max(s for s in range(STAGES) if TILE_OFFSET[s] <= w)
        g, e = int(got[wg][w]), int(want[wg][w])
        out.update(first_bad_wg=wg, first_bad_stage=stage, first_bad_word=w - TILE_OFFSET[stage],
                   first_bad_got=g, first_bad_want=e, first_bad_xor=g ^ e)
    return out


def assert_verdict(got: dict, want: dict, what: str = "") -> None:
    """`got`: a parsed datapath_bf16_json line; `want`: verdict(). Every field of
    `want` equal in type and value."""
    for key, w in want.items():
        assert key in got, f"{what}: no {key!r} in {sorted(got)}"
        assert type(got[key]) is type(w) and got[key] == w, f"{what}: {key} {got[key]!r} want {w!r}"


# ---- native/tests/datapath_bf16_contract_cli.cpp --------------------------------------
RECORDS, TILES = 0, 1      # a patch's array


def compile_cli(exe, extra_flags=()) -> Path:
    from .contract_cli import host_compiler
    cxx = host_compiler()
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", *extra_flags]
    for inc in CLI_INCLUDES:
        cmd += ["-I", str(inc)]
    subprocess.run(cmd + [str(CLI_SOURCE), "-o", str(exe)], check=True, timeout=300)
    return Path(exe)


def contract_cli(build_dir) -> Path:
    """The program the native build left in the package's bin directory when it
    was built from the sources as they are now, else one compiled into `build_dir`."""
    from .. import _build
    from .contract_cli import host_compiler
    exe = _build.DATAPATH_BF16_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "datapath_bf16_contract_cli")


def case(records, tiles, grid: int, nonce: int, variants=()) -> bytes:
    """One `verdict` case; a variant is a list of (array, index, value) word replacements."""
    records = np.ascontiguousarray(records, dtype=np.uint32)
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
    assert records.size == grid * REC_WORDS and tiles.size == grid * WG_WORDS, (records.size, tiles.size, grid)
    blob = [struct.pack("<III", grid, nonce, len(variants)), records.tobytes(), tiles.tobytes()]
    for patches in variants:
        flat = np.asarray([tuple(int(x) & M32 for x in p) for p in patches], dtype=np.uint32).reshape(-1, 3)
        blob.append(struct.pack("<I", len(flat)) + flat.tobytes())
    return b"".join(blob)


def run_cli(cli, command: str, blob: bytes, expect: int, timeout: float = 300) -> list:
    r = subprocess.run([str(cli), command], input=blob, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    lines = r.stdout.decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == expect, (len(lines) - 1, expect)
    return lines[:-1]


def verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_cli(cli, "verdict", b"".join(blobs), expect)]
