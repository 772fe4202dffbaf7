"""Independent reference for the f16 MFMA datapath check
(mi355x_mfma_datapath_f16, native/src/health/datapath_f16_kernel.h,
datapath_f16_verify.h).

Written from the recipe in the header's comment, in Python integers: a number
is a pair (m, e) standing for m * 2^e, a product multiplies the m and adds the
e, a sum aligns to the smallest e. Nothing here rounds: `f32_word` refuses a
value that is not exactly an f32, and `terms` / `quantum` hand the tests what
they need to show that no partial sum, in any order, can need more than 24
bits.

Also: the record / tile image a correct kernel writes, the verdict the host
draws from them, wrong-kernel and stuck-bit models (those do round, to nearest
even, since a wrong kernel's sums need not be exact), and a driver for
native/tests/datapath_f16_contract_cli.cpp.
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
CLI_SOURCE = REPO / "native" / "tests" / "datapath_f16_contract_cli.cpp"
CLI_INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

M32 = 0xFFFFFFFF
STAGES = 7
# per stage: 32x32x16 (four times), 16x16x32, 32x32x8, 16x16x16
DIM = (32, 32, 32, 32, 16, 32, 16)      # rows = columns of a stage's tile
BLOCKS = (2, 2, 2, 2, 4, 2, 4)          # K-blocks (lane groups) of a stage's instruction
DWORDS = (4, 4, 4, 4, 4, 2, 2)          # dwords a lane hands the instruction: 8 halves, legacy forms 4
DEPTH = tuple(2 * d * b for d, b in zip(DWORDS, BLOCKS))   # K: 16, 16, 16, 16, 32, 8, 16
TILE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = (0, 1024, 2048, 3072, 4096, 4352, 5376)
WG_WORDS = 5 * 1024 + 2 * 256
REC_WORDS = 16
WAVES = 4
THREADS = 256
MAGIC = int.from_bytes(b"DPHF", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8

GOLDEN, MURMUR = 0x9E3779B1, 0x85EBCA77
SEL_A, SEL_B, SEL_C, SEL_HOT, SEL_ROT, SEL_EA, SEL_EB = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800, 0x3900, 0x3A00
BAND = range(1, 31)                 # exponent fields of an f16 band half
ONE_HOT_A, ONE_HOT_B = (1,), (0, 2)  # the stages whose A / B operand is one-hot
ONE_HOT_STAGES = (0, 1, 2)
FULL_HOT = (2,)                     # the hot element is a band half, not a power of two
SUM_STAGES = (3, 4, 5, 6)
NARROW_A = (4, 6)                   # A narrow and B full odd; stages 3 and 5 the other way round
GA_LIMIT = 1 << 21                  # |ga| of C = ga * q


# ---- integer hashes ---------------------------------------------------------------
def wave_nonce(nonce: int, wg: int, wave: int) -> int:
    return ((nonce ^ wg * GOLDEN & M32) + wave * MURMUR) & M32


def mix(nw: int, stage: int, selector: int) -> int:
    h = nw ^ ((stage + 0x51) * GOLDEN & M32) ^ (selector * MURMUR & M32)
    for shift, mult in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h ^= h >> shift
        h = h * mult & M32
    return h ^ h >> 16


# ---- numbers: (m, e) is m * 2^e --------------------------------------------------
def f16_value(h: int) -> tuple:
    """An IEEE half: +-(1024 + m) * 2^(E - 25); the recipe's only other pattern is +0."""
    sign, e, m = h >> 15, h >> 10 & 0x1F, h & 0x3FF
    assert e != 31, hex(h)
    mag, exp = (m, -24) if e == 0 else (1024 + m, e - 25)
    return (-mag if sign else mag, exp)


def bf16_value(h: int) -> tuple:
    """The same 16 bits read as bf16 (a wrong-kernel model)."""
    sign, e, m = h >> 15, h >> 7 & 0xFF, h & 0x7F
    if e == 255:
        e = 254                                   # the model has no Inf / NaN: the largest finite binade
    mag, exp = (m, -133) if e == 0 else (128 + m, e - 134)
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


def widen(h: int) -> int:
    """The header's integer widening of a half to the f32 word of the same value."""
    sign = (h & 0x8000) << 16
    if h & 0x7FFF == 0:
        return sign
    return sign | ((h >> 10 & 0x1F) + 112) << 23 | (h & 0x3FF) << 13


def halves(word: int) -> tuple:
    """The two 16-bit elements of a fragment dword, the even element first."""
    return word & 0xFFFF, word >> 16


def in_band(h: int) -> bool:
    return (h >> 10 & 0x1F) in BAND


# ---- operand words ------------------------------------------------------------------
def band16(h16: int) -> int:
    return (h16 & 0x83FF) | (BAND[0] + ((h16 >> 10 & 0x1F) * len(BAND) >> 5)) << 10


def _band(nw: int, stage: int, selector: int, rc: int, block: int, dword: int) -> int:
    """Band halves; dword 1 is the complement of dword 0, dword 3 of dword 2."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 4 + dword // 2 * 2)
    w = band16(h & 0xFFFF) | band16(h >> 16) << 16
    return w ^ M32 if dword % 2 else w


def onehot_position(stage: int, rc: int, nw: int) -> int:
    """The k (0..15) where row / column `rc` of a one-hot operand is not zero."""
    return (rc + mix(nw, stage, SEL_ROT) % 16) % 16


def onehot_entry(stage: int, rc: int, nw: int) -> int:
    """The f16 pattern there: +-2^f (stages 0, 1), a band half (stage 2)."""
    h = mix(nw, stage, SEL_HOT + rc)
    if stage in FULL_HOT:
        return band16(h >> 16)
    return (h >> 31) << 15 | (BAND[0] + (h & 0xFFFF) % len(BAND)) << 10


def _onehot(nw: int, stage: int, rc: int, block: int, dword: int) -> int:
    pos = onehot_position(stage, rc, nw)
    if pos // 2 != block * 4 + dword:
        return 0
    return onehot_entry(stage, rc, nw) << 16 * (pos % 2)


def exponent_field(nw: int, stage: int, selector: int, rc: int) -> int:
    return BAND[0] + mix(nw, stage, selector + rc) % len(BAND)


def _odd(nw: int, stage: int, selector: int, rc: int, block: int, dword: int, e: int, narrow: bool) -> int:
    """Two full odd elements +-(1024 + m) * 2^(e - 25), m odd; or two narrow ones
    +-(32 + m') * 2^(e - 20), m' odd: mantissa bits 5..9 only, bit 5 set."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 4 + dword)
    w = (h & 0x83E083E0) | 0x00200020 if narrow else (h & 0x83FF83FF) | 0x00010001
    return w | e << 10 | e << 26


def a_word(stage: int, row: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_A:
        return _onehot(nw, stage, row, block, dword)
    if stage in SUM_STAGES:
        return _odd(nw, stage, SEL_A, row, block, dword, exponent_field(nw, stage, SEL_EA, row), stage in NARROW_A)
    return _band(nw, stage, SEL_A, row, block, dword)


def b_word(stage: int, col: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_B:
        return _onehot(nw, stage, col, block, dword)
    if stage in SUM_STAGES:
        return _odd(nw, stage, SEL_B, col, block, dword, exponent_field(nw, stage, SEL_EB, col),
                    stage not in NARROW_A)
    return _band(nw, stage, SEL_B, col, block, dword)


def quantum(stage: int, row: int, col: int, nw: int) -> int:
    """Stages 3..6: the exponent x of q = 2^x, of which C and every product of D[row][col] are multiples."""
    return exponent_field(nw, stage, SEL_EA, row) + exponent_field(nw, stage, SEL_EB, col) - 45


def c_word(stage: int, row: int, col: int, nw: int) -> int:
    if stage in SUM_STAGES:
        h = mix(nw, stage, SEL_C + 32 * row + col)
        ga = (h & (GA_LIMIT - 1)) | 1
        return f32_word((-ga if h >> 31 else ga, quantum(stage, row, col, nw)))
    return 0


@lru_cache(maxsize=None)
def operands(stage: int, nw: int):
    """(A words [dim][blocks*dwords], B words [dim][blocks*dwords], C words [dim][dim]) of one
    wave's stage; operand word block*dwords + dword of a row / column holds k = 2 * word and 2 * word + 1."""
    dim, dw = DIM[stage], DWORDS[stage]
    words = BLOCKS[stage] * dw
    a = tuple(tuple(a_word(stage, i, w // dw, w % dw, nw) for w in range(words)) for i in range(dim))
    b = tuple(tuple(b_word(stage, j, w // dw, w % dw, nw) for w in range(words)) for j in range(dim))
    c = tuple(tuple(c_word(stage, i, j, nw) for j in range(dim)) for i in range(dim))
    return a, b, c


def elements(fragment) -> list:
    """The 16-bit patterns of a row / column in k order."""
    return [h for word in fragment for h in halves(word)]


def _values(fragment, decode=f16_value) -> list:
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
    """Per operand, the bits that take both values in every single fragment (the
    four dwords one lane hands the instruction) of A in stage 0 and of B in stage 1."""
    a0, _, _ = operands(0, nw)
    _, b1, _ = operands(1, nw)

    def every(groups) -> int:
        out = M32
        for g in groups:
            out &= _both(g)
        return out

    def fragments(rows) -> list:
        return [row[4 * h:4 * h + 4] for row in rows for h in range(len(row) // 4)]
    return {"A": every(fragments(a0)), "B": every(fragments(b1))}


def selected_positions(stage: int, nw: int) -> list:
    """Stages 0..2: per column / row, the k its one-hot entry selects, read back
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
    """tiles[wg][5632] as uint32: wave 0's seven tiles of every workgroup, five
    of 32x32 and two of 16x16. Computed once per (nonce, grid) and read-only:
    copy before changing it."""
    key = (nonce, grid)
    if key not in _tiles_cache:
        t = np.array([[w for s in range(STAGES) for w in expected_tile(s, wave_nonce(nonce, wg, 0))]
                      for wg in range(grid)], dtype=np.uint32).reshape(grid, WG_WORDS)
        t.setflags(write=False)
        _tiles_cache[key] = t
    return _tiles_cache[key]


def stage_of_word(word: int) -> int:
    """The stage whose tile holds word `word` of a workgroup's tiles."""
    return max(s for s in range(STAGES) if TILE_OFFSET[s] <= word)


def spread_placement(grid: int, xcds: int = 8) -> list:
    """(xcc, cu-bits) per workgroup: dealt round-robin to the XCDs."""
    return [(wg % xcds, wg // xcds) for wg in range(grid)]


def healthy(grid: int, nonce: int, placement=None, tiles=None):
    """(records, tiles) a correct mi355x_mfma_datapath_f16 would write; wave v of
    a workgroup on SIMD v of its CU. `tiles`: an image got elsewhere (header_tiles), copied."""
    placement = list(placement or spread_placement(grid))
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        recs[wg, REC_MAGIC], recs[wg, REC_WG], recs[wg, REC_NONCE], recs[wg, REC_XCC] = MAGIC, wg, nonce ^ wg, xcc
        for v in range(WAVES):
            recs[wg, REC_HWID + v] = cu << 8 | v << 4 | 0x1
    return recs, (tiles_image(nonce, grid) if tiles is None else np.asarray(tiles, dtype=np.uint32)).copy()


ACC_REGS = (16, 16, 16, 16, 4, 16, 4)
INDEX_STRIDE = 16                   # inject index = stage * 16 + register


def accumulator_element(stage: int, lane: int, reg: int) -> tuple:
    """(row, column) of the stage's tile that accumulator register `reg` of lane
    `lane` holds: 32x32: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]; 16x16: D[4*(l>>4) + r][l&15]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS[stage]
    if DIM[stage] == 16:
        return 4 * (lane >> 4) + reg, lane & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def injection_image(nonce: int, grid: int, inject=None) -> tuple:
    """(stage_bad (grid, 7), tiles (grid, 5632) uint32) that
    mi355x_mfma_datapath_f16 of the test-only build must leave behind under
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


def _blocks_swapped(words, stage: int) -> list:
    dw = DWORDS[stage]
    blocks = [words[k:k + dw] for k in range(0, len(words), dw)]
    return [w for blk in blocks[1:] + blocks[:1] for w in blk]


def _halves_swapped(words, stage: int) -> list:
    """The two halves of every dword exchanged."""
    return [(w >> 16 | w << 16) & M32 for w in words]


def _legacy_as_x16(words, stage: int) -> list:
    """A filled as if lane group h of a legacy form held k = 8h + e, like the x16 / x32 forms, instead of
    4h + e: group h gets the elements that belong to group 2h (mod the groups). The other stages unchanged."""
    dw, blocks = DWORDS[stage], BLOCKS[stage]
    if dw == 4:
        return words
    return [w for h in range(blocks) for w in words[(2 * h % blocks) * dw:(2 * h % blocks) * dw + dw]]


def _low_mantissa_dropped(words, stage: int) -> list:
    """Mantissa bits 0..2 of every half read as zero."""
    return [w & 0xFFF8FFF8 for w in words]


def _top16(product: tuple) -> tuple:
    m, e = product
    drop = max(abs(m).bit_length() - 16, 0)
    return ((abs(m) >> drop << drop) * (-1 if m < 0 else 1), e)


def _model(nw: int, stage: int, fix_a=None, fix_b=None, fix_c=None, decode=f16_value, fix_product=None) -> list:
    """A stage's tile with a change applied to A's words, B's words, C's word,
    the decoding or each product; rounded to nearest even where it is not exact."""
    a, b, c = operands(stage, nw)
    dim = DIM[stage]
    av = [_values(fix_a(list(f), stage) if fix_a else f, decode) for f in a]
    bv = [_values(fix_b(list(f), stage) if fix_b else f, decode) for f in b]
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
            out.append(f32_round(total(([f32_value(cw)] if cw is not None else [(0, 0)]) + prods)))
    return out


STUCK_MODELS = {"A bit 17 stuck at 0": ("a", 17, 0), "B bit 2 stuck at 1": ("b", 2, 1), "C bit 12 stuck at 1": ("c", 12, 1),
                "D bit 30 stuck at 0": ("d", 30, 0)}


def wrong_kernel_models(nonce: int, grid: int) -> dict:
    """Tile images of kernels (or of a unit) that get the instruction's contract wrong."""
    good = tiles_image(nonce, grid)

    def rebuilt(**how):
        return np.array([[w for s in range(STAGES) for w in _model(wave_nonce(nonce, wg, 0), s, **how)]
                         for wg in range(grid)], dtype=np.uint32).reshape(good.shape)

    out = {
        "halves of A's dwords swapped": rebuilt(fix_a=_halves_swapped),
        "A's K-blocks of the lane groups swapped": rebuilt(fix_a=_blocks_swapped),
        "A of the legacy forms laid out by the x16 k-map": rebuilt(fix_a=_legacy_as_x16),
        "operands decoded as bf16": rebuilt(decode=bf16_value),
        "mantissa bits 0..2 of A and B dropped": rebuilt(fix_a=_low_mantissa_dropped, fix_b=_low_mantissa_dropped),
        "products truncated to their top 16 bits": rebuilt(fix_product=_top16),
        "C dropped": rebuilt(fix_c=lambda w: None),
    }
    for name, (what, bit, value) in STUCK_MODELS.items():
        if what == "d":
            out[name] = stuck_bit(good, bit, value)
        elif what == "c":
            out[name] = rebuilt(fix_c=lambda w: _stuck_words([w], bit, value)[0])
        else:
            out[name] = rebuilt(**{"fix_" + what: lambda ws, stage: _stuck_words(ws, bit, value)})
    return out


# ---- the verdict (datapath_f16_verify.h), from the field comments of mi355x_datapath_f16_result ----
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
    """`got`: a parsed datapath_f16_json line; `want`: verdict(). Every field of
    `want` equal in type and value."""
    for key, w in want.items():
        assert key in got, f"{what}: no {key!r} in {sorted(got)}"
        assert type(got[key]) is type(w) and got[key] == w, f"{what}: {key} {got[key]!r} want {w!r}"


# ---- native/tests/datapath_f16_contract_cli.cpp --------------------------------------
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
    exe = _build.DATAPATH_F16_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "datapath_f16_contract_cli")


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


def header_tiles(cli, nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][5632] as datapath_f16_verify.h expects them (the contract program's `tile` requests): for a
    grid too large to compute in Python integers in a test's time. tests/test_native_datapath_f16.py holds
    the header's tiles to the reference word for word."""
    lines = [f"tile {s} {wave_nonce(nonce, wg, 0)}" for wg in range(grid) for s in range(STAGES)]
    out = run_cli(cli, "gen", ("\n".join(lines) + "\n").encode(), len(lines))
    return np.array([int(x) for ln in out for x in ln.split()], dtype=np.uint32).reshape(grid, WG_WORDS)


def verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_cli(cli, "verdict", b"".join(blobs), expect)]
