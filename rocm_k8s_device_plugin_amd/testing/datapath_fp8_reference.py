"""Independent reference for the fp8 / MX-scaled MFMA datapath check
(mi355x_mfma_datapath_fp8, native/src/health/datapath_fp8_kernel.h,
datapath_fp8_verify.h).

Written from the recipe in the header's comment, in Python integers: an fp8
byte is (sign, m, e) fields, a number is a pair (m, e) standing for m * 2^e, a
product multiplies the m and adds the e (an E8M0 scale byte s adds s - 127), a
sum aligns to the smallest e. Nothing here rounds: `f32_word` refuses a value
that is not exactly a normal f32, and `terms` / `quantum` hand the tests what
they need to show that no partial sum, in any order, can need more than 24
bits. The arithmetic on (m, e) pairs is datapath_bf16_reference's.

Also: the record / tile image a correct kernel writes, the verdict the host
draws from them, wrong-kernel and stuck-bit models (those do round, to nearest
even, since a wrong kernel's sums need not be exact), and a driver for
native/tests/datapath_fp8_contract_cli.cpp.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np

from .datapath_bf16_reference import (assert_verdict, f32_round, f32_value, f32_word, run_cli, spread_placement,  # noqa: F401
                                      stuck_bit, total)

REPO = Path(__file__).resolve().parent.parent.parent
CLI_SOURCE = REPO / "native" / "tests" / "datapath_fp8_contract_cli.cpp"
CLI_INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

M32 = 0xFFFFFFFF
STAGES = 8
DIM = (32, 32, 32, 16, 32, 32, 32, 16)          # rows = columns of a stage's tile
BLOCKS = (2, 2, 2, 4, 2, 2, 2, 4)               # K-blocks of a stage's instruction
DWORDS = (2, 2, 2, 2, 8, 8, 8, 8)               # dwords of one fragment (one lane's part of a row / column)
DEPTH = tuple(4 * b * d for b, d in zip(BLOCKS, DWORDS))   # K: 16, 16, 16, 32, 64, 64, 64, 128
E4M3, E5M2 = 0, 1
FMT_A = (E4M3, E5M2, E4M3, E5M2, E4M3, E5M2, E4M3, E5M2)
FMT_B = (E4M3, E5M2, E5M2, E4M3, E5M2, E4M3, E4M3, E5M2)
SCALED_STAGES = (4, 5, 6, 7)
ONE_HOT_A, ONE_HOT_B = (1, 5), (0, 4)           # the stages whose A / B operand is one-hot
ONE_HOT_STAGES = (0, 1, 4, 5)
PRODUCT_STAGES = (2, 3, 6, 7)
SCALE_SEL = {s: (s - 4, 7 - s) for s in SCALED_STAGES}   # the byte of the scale VGPR taken for A, for B
TILE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = tuple(sum(TILE_WORDS[:s]) for s in range(STAGES))
WG_WORDS = sum(TILE_WORDS)
REC_WORDS = 16
WAVES = 4
THREADS = 256
MAGIC = int.from_bytes(b"DPF8", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8

GOLDEN, MURMUR = 0x9E3779B1, 0x85EBCA77
SEL_A, SEL_B, SEL_C, SEL_SIGN, SEL_ROT, SEL_EA, SEL_EB = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800, 0x3900, 0x3A00
SEL_SCALE = (0x4000, 0x4800)
SEL_SBASE = (0x5000, 0x5100)
EXP_BAND = (range(1, 15), range(1, 31))         # exponent fields of a band byte, per format
MANT_BITS = (3, 2)
EXP_OFFSET = (10, 17)                           # a normal value is (2^mant_bits + m) * 2^(E - offset)
SCALE_BAND = range(97, 159)                     # E8M0 scale band bytes
SCALE_BASE = range(112, 143)                    # SA_i, SB_j of stages 6 and 7


# ---- integer hashes ---------------------------------------------------------------
def wave_nonce(nonce: int, wg: int, wave: int) -> int:
    return ((nonce ^ wg * GOLDEN & M32) + wave * MURMUR) & M32


def mix(nw: int, stage: int, selector: int) -> int:
    h = nw ^ ((stage + 0x41) * GOLDEN & M32) ^ (selector * MURMUR & M32)
    for shift, mult in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h ^= h >> shift
        h = h * mult & M32
    return h ^ h >> 16


# ---- numbers ----------------------------------------------------------------------
def fields(byte: int, fmt: int) -> tuple:
    """(sign, m, e) of an fp8 byte."""
    mb = MANT_BITS[fmt]
    return byte >> 7, byte & ((1 << mb) - 1), (byte & 0x7F) >> mb


def fp8_value(byte: int, fmt: int, bias_shift: int = 0) -> tuple:
    """(m, e) of an OCP fp8 byte; `bias_shift` 1 reads it with the fnuz bias (a wrong-kernel model)."""
    sign, m, e = fields(byte, fmt)
    mb = MANT_BITS[fmt]
    assert not (fmt == E5M2 and e == 31) and not (fmt == E4M3 and e == 15 and m == 7), hex(byte)
    mag, exp = (m, 1 - EXP_OFFSET[fmt]) if e == 0 else ((1 << mb) + m, e - EXP_OFFSET[fmt])
    return (-mag if sign else mag, exp - bias_shift)


def in_band(byte: int, fmt: int) -> bool:
    return fields(byte, fmt)[2] in EXP_BAND[fmt]


def byte_list(words) -> list:
    """The bytes of a row / column in k order."""
    return [w >> 8 * e & 0xFF for w in words for e in range(4)]


# ---- operand words ------------------------------------------------------------------
def band8(h8: int, fmt: int) -> int:
    if fmt == E5M2:
        return (h8 & 0x83) | (1 + ((h8 >> 2 & 0x1F) * 30 >> 5)) << 2
    return (h8 & 0x87) | (1 + ((h8 >> 3 & 0xF) * 14 >> 4)) << 3


def _band(nw: int, stage: int, selector: int, fmt: int, rc: int, block: int, dword: int) -> int:
    """Band bytes; each odd dword is the complement of the even dword before it."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 8 + dword // 2 * 2)
    w = sum(band8(h >> 8 * e & 0xFF, fmt) << 8 * e for e in range(4))
    return w ^ M32 if dword % 2 else w


def onehot_position(stage: int, rc: int, nw: int) -> int:
    """The (block, byte) position where row / column `rc` of a one-hot operand is not zero."""
    if stage in SCALED_STAGES:
        return (rc + 16 * (nw & 3)) % 64
    return (rc + mix(nw, stage, SEL_ROT) % 16) % 16


def onehot_entry(stage: int, fmt: int, rc: int, nw: int) -> int:
    """The byte of +-2^f there."""
    h = mix(nw, stage, SEL_SIGN + rc)
    return (h >> 31) << 7 | (1 + (h & 0xFFFF) % len(EXP_BAND[fmt])) << MANT_BITS[fmt]


def _onehot(nw: int, stage: int, fmt: int, rc: int, block: int, dword: int) -> int:
    pos = onehot_position(stage, rc, nw)
    if pos // 4 != block * DWORDS[stage] + dword:
        return 0
    return onehot_entry(stage, fmt, rc, nw) << 8 * (pos % 4)


def exponent_field(nw: int, stage: int, selector: int, fmt: int, rc: int) -> int:
    return 1 + mix(nw, stage, selector + rc) % len(EXP_BAND[fmt])


def _odd(nw: int, stage: int, selector: int, fmt: int, rc: int, block: int, dword: int, e: int) -> int:
    """Four elements with any sign, an odd mantissa and exponent field e."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 8 + dword)
    if fmt == E5M2:
        return (h & 0x83838383) | 0x01010101 | e * 0x04040404
    return (h & 0x87878787) | 0x01010101 | e * 0x08080808


def a_word(stage: int, row: int, block: int, dword: int, nw: int) -> int:
    fmt = FMT_A[stage]
    if stage in ONE_HOT_A:
        return _onehot(nw, stage, fmt, row, block, dword)
    if stage in PRODUCT_STAGES:
        return _odd(nw, stage, SEL_A, fmt, row, block, dword, exponent_field(nw, stage, SEL_EA, fmt, row))
    return _band(nw, stage, SEL_A, fmt, row, block, dword)


def b_word(stage: int, col: int, block: int, dword: int, nw: int) -> int:
    fmt = FMT_B[stage]
    if stage in ONE_HOT_B:
        return _onehot(nw, stage, fmt, col, block, dword)
    if stage in PRODUCT_STAGES:
        return _odd(nw, stage, SEL_B, fmt, col, block, dword, exponent_field(nw, stage, SEL_EB, fmt, col))
    return _band(nw, stage, SEL_B, fmt, col, block, dword)


def scale_base(nw: int, stage: int, which: int, rc: int) -> int:
    return SCALE_BASE[0] + mix(nw, stage, SEL_SBASE[which] + rc) % len(SCALE_BASE)


def scale_offset(nw: int, stage: int, which: int, rc: int, block: int) -> int:
    """d (which = 0) or d' (which = 1) of stages 6 and 7, per row / column and scale block."""
    return mix(nw, stage, SEL_SCALE[which] + rc * 4 + block) & 3


def scale_byte(nw: int, stage: int, which: int, rc: int, block: int) -> int:
    if stage in PRODUCT_STAGES:
        return scale_base(nw, stage, which, rc) + scale_offset(nw, stage, which, rc, block)
    return SCALE_BAND[0] + mix(nw, stage, SEL_SCALE[which] + rc * 4 + block) % len(SCALE_BAND)


def scale_word(nw: int, stage: int, which: int, rc: int, block: int) -> int:
    """The scale VGPR of lane (rc, lane group `block`), which holds the scale of scale block
    `block` (scale_block): the scale in the selected byte, three more band values, all four different, in the rest."""
    s = scale_byte(nw, stage, which, rc, block) - SCALE_BAND[0]
    sel = SCALE_SEL[stage][which]
    return sum((SCALE_BAND[0] + (s + (p - sel) % 4 * 15) % len(SCALE_BAND)) << 8 * p for p in range(4))


def quantum(stage: int, row: int, col: int, nw: int) -> int:
    """Product stages: the exponent x of q = 2^x, of which C and every product of D[row][col] are multiples."""
    fa, fb = FMT_A[stage], FMT_B[stage]
    x = (exponent_field(nw, stage, SEL_EA, fa, row) + exponent_field(nw, stage, SEL_EB, fb, col)
         - EXP_OFFSET[fa] - EXP_OFFSET[fb])
    if stage in SCALED_STAGES:
        x += scale_base(nw, stage, 0, row) + scale_base(nw, stage, 1, col) - 254
    return x


def c_word(stage: int, row: int, col: int, nw: int) -> int:
    if stage not in PRODUCT_STAGES:
        return 0
    h = mix(nw, stage, SEL_C + 32 * row + col)
    ga = (h & 0xFFFFF) | 1
    return f32_word((-ga if h >> 31 else ga, quantum(stage, row, col, nw)))


@lru_cache(maxsize=None)
def operands(stage: int, nw: int):
    """(A words [dim][blocks*dwords], B words likewise, C words [dim][dim], A's scale
    VGPRs [dim][blocks] or None, B's likewise) of one wave's stage; word block * dwords
    + dword of a row / column holds k = 4 * word .. 4 * word + 3."""
    dim, dw = DIM[stage], DWORDS[stage]
    words = BLOCKS[stage] * dw
    a = tuple(tuple(a_word(stage, i, w // dw, w % dw, nw) for w in range(words)) for i in range(dim))
    b = tuple(tuple(b_word(stage, j, w // dw, w % dw, nw) for w in range(words)) for j in range(dim))
    c = tuple(tuple(c_word(stage, i, j, nw) for j in range(dim)) for i in range(dim))
    sa = sb = None
    if stage in SCALED_STAGES:
        sa, sb = (tuple(tuple(scale_word(nw, stage, which, rc, h) for h in range(BLOCKS[stage])) for rc in range(dim))
                  for which in (0, 1))
    return a, b, c, sa, sb


def selected_scales(stage: int, which: int, scale_words, select=None) -> list:
    """Per row / column and block, the byte the stage selects from the scale VGPR (127, no scale, when not scaled)."""
    if scale_words is None:
        return [[127] * BLOCKS[stage] for _ in range(DIM[stage])]
    sel = SCALE_SEL[stage][which] if select is None else select
    return [[w >> 8 * sel & 0xFF for w in row] for row in scale_words]


def scale_block(stage: int, k: int, own_fragment: bool = False) -> int:
    """The lane group whose scale applies to byte `k` of a row / column (bytes in the order the lanes hold
    them: lane group k // 32, byte k % 32 of its fragment). Measured on an MI355X: not the group's own
    (`own_fragment`, the refuted assumption, kept as a wrong-kernel model) but one 16-byte half of two
    groups' fragments: 32x32x64 half e // 16; 16x16x128 2 * (e // 16) + group // 2."""
    if stage not in SCALED_STAGES:
        return k // (4 * DWORDS[stage])
    group, e = divmod(k, 32)
    if own_fragment:
        return group
    return 2 * (e // 16) + group // 2 if DIM[stage] == 16 else e // 16


def _values(fragment, fmt: int, scales, stage: int, decode=fp8_value, own_fragment=False) -> list:
    """The elements of a row / column as (m, e), each with its scale block's scale applied."""
    out = []
    for k, byte in enumerate(byte_list(fragment)):
        m, e = decode(byte, fmt)
        out.append((m, e + scales[scale_block(stage, k, own_fragment)] - 127))
    return out


def terms(stage: int, nw: int, row: int, col: int) -> list:
    """C and the K products of D[row][col], each as (m, e)."""
    a, b, c, sa, sb = operands(stage, nw)
    av = _values(a[row], FMT_A[stage], selected_scales(stage, 0, sa)[row], stage)
    bv = _values(b[col], FMT_B[stage], selected_scales(stage, 1, sb)[col], stage)
    return [f32_value(c[row][col])] + [(x * y, ex + ey) for (x, ex), (y, ey) in zip(av, bv)]


def _tile(stage: int, a, b, c, sa_sel, sb_sel, exact: bool, decode_a=fp8_value, decode_b=fp8_value,
          fmt_a=None, fmt_b=None, c_scale=None, own_fragment=False) -> list:
    dim = DIM[stage]
    fa = FMT_A[stage] if fmt_a is None else fmt_a
    fb = FMT_B[stage] if fmt_b is None else fmt_b
    av = [_values(a[i], fa, sa_sel[i], stage, decode_a, own_fragment) for i in range(dim)]
    bv = [_values(b[j], fb, sb_sel[j], stage, decode_b, own_fragment) for j in range(dim)]
    out = []
    for i in range(dim):
        for j in range(dim):
            cw = c[i][j]
            parts = [(x * y, ex + ey) for (x, ex), (y, ey) in zip(av[i], bv[j])]
            if cw is not None:
                if cw >> 23 & 0xFF == 255:
                    out.append(cw)                  # an Inf or NaN in C comes out as it went in
                    continue
                m, e = f32_value(cw)
                parts.append((m, e + (c_scale(i, j) if c_scale else 0)))
            out.append(f32_word(total(parts)) if exact else f32_round(total(parts)))
    return out


@lru_cache(maxsize=None)
def expected_tile(stage: int, nw: int) -> tuple:
    """The output words of one wave's stage, row-major: C + sum over k of A * B * scales, exactly."""
    a, b, c, sa, sb = operands(stage, nw)
    return tuple(_tile(stage, a, b, c, selected_scales(stage, 0, sa), selected_scales(stage, 1, sb), exact=True))


def selected_positions(stage: int, nw: int) -> list:
    """One-hot stages: per column / row, the position its entry selects, read back from the operand words."""
    a, b, _, _, _ = operands(stage, nw)
    out = []
    for f in (b if stage in ONE_HOT_B else a):
        nz = [k for k, byte in enumerate(byte_list(f)) if byte]
        assert len(nz) == 1, (stage, f)
        out.append(nz[0])
    return out


# ---- what a correct kernel writes ----------------------------------------------------
_tiles_cache: dict = {}


def tiles_image(nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][6656] as uint32: wave 0's eight tiles of every workgroup. Computed
    once per (nonce, grid) and read-only: copy before changing it."""
    key = (nonce, grid)
    if key not in _tiles_cache:
        t = np.array([[w for s in range(STAGES) for w in expected_tile(s, wave_nonce(nonce, wg, 0))]
                      for wg in range(grid)], dtype=np.uint32).reshape(grid, WG_WORDS)
        t.setflags(write=False)
        _tiles_cache[key] = t
    return _tiles_cache[key]


def healthy(grid: int, nonce: int, placement=None, tiles=None):
    """(records, tiles) a correct mi355x_mfma_datapath_fp8 would write; wave v of a
    workgroup on SIMD v of its CU. `tiles`: an image got elsewhere (header_tiles), copied."""
    placement = list(placement or spread_placement(grid))
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        recs[wg, REC_MAGIC], recs[wg, REC_WG], recs[wg, REC_NONCE], recs[wg, REC_XCC] = MAGIC, wg, nonce ^ wg, xcc
        for v in range(WAVES):
            recs[wg, REC_HWID + v] = cu << 8 | v << 4 | 0x1
    return recs, (tiles_image(nonce, grid) if tiles is None else np.asarray(tiles, dtype=np.uint32)).copy()


ACC_REGS = tuple(16 if d == 32 else 4 for d in DIM)
INDEX_STRIDE = 16                   # inject index = stage * 16 + register


def accumulator_element(stage: int, lane: int, reg: int) -> tuple:
    """(row, column) of the stage's tile that accumulator register `reg` of lane
    `lane` holds: 32x32: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]; 16x16: D[4*(l>>4) + r][l&15]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS[stage]
    if DIM[stage] == 16:
        return 4 * (lane >> 4) + reg, lane & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def injection_image(nonce: int, grid: int, inject=None) -> tuple:
    """(stage_bad (grid, 8), tiles (grid, 6656) uint32) that mi355x_mfma_datapath_fp8
    of the test-only build must leave behind under `inject` (a raw_kernels
    request's "inject" object: index = stage * 16 + register; None for the hook
    off), from the documented layout alone. The wrong word is counted once, by
    its workgroup, in its stage's counter; it reaches the host's tiles only from
    wave 0, and there it differs from the healthy word by exactly the mask. An
    index that names no register injects nothing."""
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


def stage_of_word(w: int) -> int:
    return max(s for s in range(STAGES) if TILE_OFFSET[s] <= w)


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
        stage = stage_of_word(w)
        per_stage = [int(((bad[:, 1] >= TILE_OFFSET[s]) & (bad[:, 1] < TILE_OFFSET[s] + TILE_WORDS[s])).sum())
                     for s in range(STAGES)]
        raise AssertionError(f"nonce {nonce:#x} grid {grid}: {len(bad)} tile words differ (per stage {per_stage}), "
                             f"first wg {wg} stage {stage} word {w - TILE_OFFSET[stage]}: got {int(til[wg, w]):#010x} "
                             f"want {int(want_tiles[wg, w]):#010x}")
    keep = [w for w in range(REC_WORDS) if w not in HW_WORDS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, inject, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all(), rec[:, REC_XCC].tolist()
    assert (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec[:, REC_HWID:REC_HWID + WAVES].tolist()


# ---- fault and wrong-kernel models (on the tile image) ------------------------------
def _stuck_words(words, bit: int, value: int) -> tuple:
    return tuple(w | 1 << bit if value else w & ~(1 << bit) & M32 for w in words)


def _stuck_value(byte: int, fmt: int, bias_shift: int = 0) -> tuple:
    """fp8_value for bytes a stuck bit may have pushed out of the band: an Inf or
    NaN encoding reads as the largest finite magnitude here (the model only has to differ)."""
    sign, m, e = fields(byte, fmt)
    if (fmt == E5M2 and e == 31) or (fmt == E4M3 and e == 15 and m == 7):
        byte = (byte & 0x80) | (0x7B if fmt == E5M2 else 0x7E)
    return fp8_value(byte, fmt, bias_shift)


def _model(nw: int, stage: int, fix_a=None, fix_b=None, fix_c=None, fix_scale=None, swap_formats=False,
           bias_shift=0, select_shift=0, scale_lane=0, no_scale=False, scale_c=False, swap_blocks=False,
           own_fragment=False) -> list:
    """A stage's tile with a change applied to A's or B's fragments, C's word, the
    scale VGPRs, the decoding or the scale's source; rounded to nearest even where it is not exact."""
    a, b, c, sa, sb = operands(stage, nw)
    dw = DWORDS[stage]
    if swap_blocks:
        a = tuple(row[dw:] + row[:dw] for row in a)
    if fix_a:
        a = tuple(tuple(w for h in range(BLOCKS[stage]) for w in fix_a(row[h * dw:(h + 1) * dw])) for row in a)
    if fix_b:
        b = tuple(tuple(w for h in range(BLOCKS[stage]) for w in fix_b(col[h * dw:(h + 1) * dw])) for col in b)
    if fix_c:
        c = tuple(tuple(fix_c(w) for w in row) for row in c)
    if fix_scale and sa is not None:
        sa, sb = (tuple(_stuck_words(row, *fix_scale) for row in s) for s in (sa, sb))
    sels = []
    for which, s in ((0, sa), (1, sb)):
        select = None if s is None else (SCALE_SEL[stage][which] + select_shift) % 4
        sel = selected_scales(stage, which, None if no_scale else s, select)
        if scale_lane:
            sel = [sel[rc ^ scale_lane] for rc in range(len(sel))]
        sels.append(sel)
    fa, fb = (FMT_A[stage], FMT_B[stage])
    if swap_formats:
        fa, fb = 1 - fa, 1 - fb

    def decode(byte, fmt):
        return _stuck_value(byte, fmt, bias_shift)
    c_scale = (lambda i, j: sels[0][i][0] + sels[1][j][0] - 254) if scale_c else None
    return _tile(stage, a, b, c, sels[0], sels[1], exact=False, decode_a=decode, decode_b=decode, fmt_a=fa, fmt_b=fb,
                 c_scale=c_scale, own_fragment=own_fragment)


def _bytes_reversed(fragment) -> tuple:
    """Byte e of a fragment where byte n-1-e belongs."""
    by = byte_list(fragment)[::-1]
    return tuple(sum(by[4 * d + e] << 8 * e for e in range(4)) for d in range(len(fragment)))


STUCK_MODELS = {"A bit 20 stuck at 0": dict(fix_a=lambda f: _stuck_words(f, 20, 0)),
                "B bit 5 stuck at 1": dict(fix_b=lambda f: _stuck_words(f, 5, 1)),
                "scale bit 2 stuck at 1": dict(fix_scale=(2, 1)),
                "scale bit 27 stuck at 0": dict(fix_scale=(27, 0)),
                "C bit 12 stuck at 1": dict(fix_c=lambda w: w | 1 << 12),
                "D bit 30 stuck at 0": None}


def wrong_kernel_models(nonce: int, grid: int) -> dict:
    """Tile images of kernels (or of a unit) that get the instructions' contract wrong."""
    good = tiles_image(nonce, grid)

    def rebuilt(**how):
        return np.array([[w for s in range(STAGES) for w in _model(wave_nonce(nonce, wg, 0), s, **how)]
                         for wg in range(grid)], dtype=np.uint32).reshape(good.shape)

    out = {
        "byte order of A's fragments reversed": rebuilt(fix_a=_bytes_reversed),
        "A's K-blocks swapped": rebuilt(swap_blocks=True),
        "e4m3 read as e5m2 and e5m2 as e4m3": rebuilt(swap_formats=True),
        "the fnuz exponent bias": rebuilt(bias_shift=1),
        "the scales ignored": rebuilt(no_scale=True),
        "the scale taken from the next byte": rebuilt(select_shift=1),
        "the scale taken from the neighbouring lane": rebuilt(scale_lane=1),
        "the scales applied to C as well": rebuilt(scale_c=True),
        "each lane's scale applied to its own fragment": rebuilt(own_fragment=True),
        "C dropped": rebuilt(fix_c=lambda w: None),
    }
    for name, how in STUCK_MODELS.items():
        out[name] = stuck_bit(good, 30, 0) if how is None else rebuilt(**how)
    return out


# ---- the verdict (datapath_fp8_verify.h), from the field comments of mi355x_datapath_fp8_result ----
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
        stage = stage_of_word(w)
        g, e = int(got[wg][w]), int(want[wg][w])
        out.update(first_bad_wg=wg, first_bad_stage=stage, first_bad_word=w - TILE_OFFSET[stage],
                   first_bad_got=g, first_bad_want=e, first_bad_xor=g ^ e)
    return out


# ---- native/tests/datapath_fp8_contract_cli.cpp ---------------------------------------
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
    exe = _build.DATAPATH_FP8_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "datapath_fp8_contract_cli")


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


def header_tiles(cli, nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][6656] as datapath_fp8_verify.h expects them (the contract program's `tile` requests): for a
    grid too large to compute in Python integers in a test's time. tests/test_native_datapath_fp8.py holds
    the header's tiles to the reference word for word."""
    lines = [f"tile {s} {wave_nonce(nonce, wg, 0)}" for wg in range(grid) for s in range(STAGES)]
    out = run_cli(cli, "gen", ("\n".join(lines) + "\n").encode(), len(lines))
    return np.array([int(x) for ln in out for x in ln.split()], dtype=np.uint32).reshape(grid, WG_WORDS)


def verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_cli(cli, "verdict", b"".join(blobs), expect)]
