"""Independent reference of the fp6 / fp4 MX-scaled MFMA datapath check (mi355x_mfma_datapath_f6f4): the operand
recipe of native/src/health/datapath_f6f4_kernel.h and the image a correct kernel writes, in Python integers. A code
is (u, x), meaning the exact fraction u * 2**x with u the signed count of its format's quanta. Nothing here goes
through the header; tests/test_native_datapath_f6f4.py holds the two equal."""
import functools

import numpy as np

M32 = 0xFFFFFFFF
STAGES, WAVES, REC_WORDS = 8, 4, 16
DIM = (32, 32, 32, 16, 32, 32, 32, 16)
STAGE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = tuple(sum(STAGE_WORDS[:s]) for s in range(STAGES))
WG_WORDS = sum(STAGE_WORDS)                    # 6656
MAGIC = int.from_bytes(b"DPF6", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8
IDX_A, IDX_B, IDX_C, IDX_HOT, IDX_EA = 0x0000, 0x1000, 0x2000, 0x3000, 0x3900
IDX_SCALE, IDX_BASE = (0x4000, 0x4800), (0x5000, 0x5100)
# format: (exponent bits, mantissa bits, bias), named by its cbsz / blgp selector
FORMATS = {0: (4, 3, 7), 2: (2, 3, 1), 3: (3, 2, 3), 4: (2, 1, 1)}
FMT = ((2, 3, 4, 4, 2, 3, 0, 4), (4, 4, 2, 3, 2, 4, 4, 4))        # of A and of B, per stage
ONEHOT = ((1, 3), (0, 2))                                        # the stages whose A / B is one-hot
DELTAS = {(4, 1): 3, (5, 1): 2}                                  # product stages: values of d / d' (4 otherwise)
PRODUCT_STAGES, SCALE_LO, SCALE_N, SBASE_LO, SBASE_N = (4, 5, 6, 7), 97, 62, 112, 31


def wave_nonce(nonce, wg, wave):
    return ((nonce ^ (wg * 0x9E3779B1 & M32)) + wave * 0x85EBCA77) & M32


def mix(nw, stage, idx):
    h = nw ^ ((stage + 0x6F) * 0x9E3779B1 & M32) ^ (idx * 0x85EBCA77 & M32)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h = (h ^ h >> shift) * mul & M32
    return h ^ h >> 16


def width(fmt):
    return 1 + FORMATS[fmt][0] + FORMATS[fmt][1]


def value(code, fmt):
    """(u, x) of a code: u quanta of 2**x. Subnormals are values like any other; there is no Inf or NaN."""
    eb, mb, bias = FORMATS[fmt]
    field, m = code >> mb & (1 << eb) - 1, code & (1 << mb) - 1
    u = (1 << mb | m) << field - 1 if field else m
    return (-u if code >> eb + mb else u), 1 - bias - mb


def onehot_pos(nw, stage, rc):
    return rc + 16 * (nw & 7) & 127 if DIM[stage] == 16 else rc + 16 * (nw & 3) & 63


def k_of(stage, side, group, e):
    """The k of element e of lane group `group`: a 6- or 4-bit fragment is 32 consecutive k, an 8-bit one two runs
    of 16 (measured on an MI355X)."""
    if width(FMT[side][stage]) == 8:
        return (DIM[stage] == 16 and 64 or 32) * (e >> 4) + 16 * group + (e & 15)
    return 32 * group + e


def elem(stage, side, rc, group, e, nw):
    """The code of element e (0..31) of the fragment of (row / column rc, lane group `group`) of A (side 0) or B (1)."""
    fmt = FMT[side][stage]
    (eb, mb, _), low = FORMATS[fmt], width(fmt) - 1
    if stage in ONEHOT[side]:
        if onehot_pos(nw, stage, rc) != k_of(stage, side, group, e):
            return 0
        h = mix(nw, stage, IDX_HOT + rc)
        p = (h & 0xFFFF) % (mb + (1 << eb) - 1)                    # +-2^p quanta: subnormal below mb
        return h >> 31 << low | (1 << p if p < mb else p - mb + 1 << mb)
    draw = e if stage in PRODUCT_STAGES else e & 15
    h8 = mix(nw, stage, (IDX_A, IDX_B)[side] + (rc * 4 + group) * 8 + (draw >> 2)) >> 8 * (draw & 3) & 0xFF
    if fmt == 0:                                                   # e4m3: the row's exponent field, 1..14
        return h8 & 0x87 | 1 + mix(nw, stage, IDX_EA + rc) % 14 << 3
    if stage in PRODUCT_STAGES:                                    # free codes: all but +-0
        return h8 >> 7 << low | 1 + ((h8 & 0x7F) * ((1 << low) - 1) >> 7)
    code = h8 >> 7 << low | 1 + ((h8 & 0x7F) * ((1 << low) - 2) >> 7)   # band codes; 16..31 complement 0..15
    return code ^ (2 << low) - 1 if e & 16 else code


def fragment(stage, side, rc, group, nw):
    """The fragment's dwords: the 32 codes as the fields of a little-endian bit stream."""
    w = width(FMT[side][stage])
    stream = sum(elem(stage, side, rc, group, e, nw) << e * w for e in range(32))
    return [stream >> 32 * d & M32 for d in range(w)]


def scale_base(stage, side, rc, nw):
    return SBASE_LO + mix(nw, stage, IDX_BASE[side] + rc) % SBASE_N if stage in PRODUCT_STAGES else SCALE_LO


def scale_byte(stage, side, rc, block, nw):
    n = DELTAS.get((stage, side), 4) if stage in PRODUCT_STAGES else SCALE_N
    return scale_base(stage, side, rc, nw) + mix(nw, stage, IDX_SCALE[side] + rc * 4 + block) % n


def quantum(stage, row, col, nw):
    """x of q = 2**x of output (row, col) of a product stage."""
    x = value(0, FMT[0][stage])[1] + value(0, FMT[1][stage])[1] - 1
    if FMT[0][stage] == 0:
        x += mix(nw, stage, IDX_EA + row) % 14
    return x + scale_base(stage, 0, row, nw) + scale_base(stage, 1, col, nw) - 254


def c_term(stage, row, col, nw):
    """C[row][col] as (ga, x): ga * 2**x; (0, 0) in the one-hot stages."""
    if stage not in PRODUCT_STAGES:
        return 0, 0
    h = mix(nw, stage, IDX_C + row * 32 + col)
    ga = h & 0xFFFFF | 1
    return (-ga if h >> 31 else ga), quantum(stage, row, col, nw)


def f32_bits(v, x):
    """The bit pattern of v * 2**x, which must be a normal f32 with at most 24 significant bits."""
    mag = abs(v)
    top = mag.bit_length() - 1
    assert mag and top - (mag & -mag).bit_length() + 1 < 24 and 0 < 127 + top + x < 255, (v, x)
    return (v < 0) << 31 | 127 + top + x << 23 | (mag << 23 >> top if top <= 23 else mag >> top - 23) & 0x7FFFFF


def operand(stage, side, nw):
    """[rc][k] -> (n, x): A[rc][k] or B[rc][k] with the scale of its scale block k >> 5 applied is n * 2**x."""
    groups = DIM[stage] == 16 and 4 or 2
    out = [[None] * (32 * groups) for _ in range(DIM[stage])]
    for rc, group, e in ((rc, g, e) for rc in range(DIM[stage]) for g in range(groups) for e in range(32)):
        k, (u, x) = k_of(stage, side, group, e), value(elem(stage, side, rc, group, e, nw), FMT[side][stage])
        out[rc][k] = (u, x + scale_byte(stage, side, rc, k >> 5, nw) - 127)
    return out


def expected_tile(stage, nw):
    a, b, words = operand(stage, 0, nw), operand(stage, 1, nw), []
    for row in range(DIM[stage]):
        for col in range(DIM[stage]):
            ts = [t for t in [c_term(stage, row, col, nw)] + [(ua * ub, xa + xb) for (ua, xa), (ub, xb) in
                                                               zip(a[row], b[col])] if t[0]]
            low = min(x for _, x in ts)
            words.append(f32_bits(sum(v << x - low for v, x in ts), low))
    return words


@functools.lru_cache(maxsize=None)
def _wg_tiles(nw):
    return tuple(w for s in range(STAGES) for w in expected_tile(s, nw))


@functools.lru_cache(maxsize=None)
def tiles_image(nonce, grid):
    """tiles[wg][6656] as uint32: wave 0's eight tiles of every workgroup. Computed once per (nonce, grid), read-only."""
    t = np.array([_wg_tiles(wave_nonce(nonce, wg, 0)) for wg in range(grid)], dtype=np.uint32)
    t.setflags(write=False)
    return t


def healthy(grid, nonce):
    """(records, tiles) of a correct kernel that found nothing; where it ran (XCC id, HW_ID words) is left zero."""
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    recs[:, :3] = [(MAGIC, wg, nonce ^ wg) for wg in range(grid)]
    return recs, tiles_image(nonce, grid).copy()


def image_bytes(records, tiles) -> bytes:
    return np.ascontiguousarray(records, dtype="<u4").tobytes() + np.ascontiguousarray(tiles, dtype="<u4").tobytes()


def compare_raw(records, tiles, nonce, grid):
    """What a launch left: (stage counts per workgroup, (wg, word) of the tile words that differ from the image)."""
    rec, (want_rec, want) = records.reshape(grid, REC_WORDS), healthy(grid, nonce)
    keep = [REC_MAGIC, REC_WG, REC_NONCE]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    return rec[:, REC_BAD:REC_BAD + STAGES], np.argwhere(tiles.reshape(grid, WG_WORDS) != want).tolist()
