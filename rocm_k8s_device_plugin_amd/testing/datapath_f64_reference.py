"""Independent reference of the f64 MFMA datapath check (mi355x_mfma_datapath_f64): the operand recipe of
native/src/health/datapath_f64_kernel.h and the image a correct kernel writes, in Python integers. A double is
(v, e), meaning v * 2**e. Nothing here goes through the header; tests/test_datapath_f64_reference.py holds the two equal."""
import functools

import numpy as np

M32, M52, M63 = 0xFFFFFFFF, (1 << 52) - 1, (1 << 63) - 1
STAGES, WAVES, REC_WORDS = 7, 4, 16
TILES = (2, 2, 1, 1, 3, 2, 1)                  # tiles of a stage
DOUBLES = (256, 256, 256, 256, 256, 64, 64)    # doubles of a tile: 16x16, or four 4x4 blocks
STAGE_WORDS = tuple(2 * t * d for t, d in zip(TILES, DOUBLES))
TILE_OFFSET = tuple(sum(STAGE_WORDS[:s]) for s in range(STAGES))
WG_WORDS = sum(STAGE_WORDS)                    # 4992
MAGIC = int.from_bytes(b"DPDF", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8
IDX_A, IDX_B, IDX_C, IDX_HOT, IDX_ROT, IDX_EA, IDX_EB = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800, 0x3900, 0x3A00
SUM_STAGES = (3, 4, 6)


def wave_nonce(nonce, wg, wave):
    return ((nonce ^ (wg * 0x9E3779B1 & M32)) + wave * 0x85EBCA77) & M32


def mix(nw, stage, idx):
    h = nw ^ ((stage + 0x64) * 0x9E3779B1 & M32) ^ (idx * 0x85EBCA77 & M32)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h = (h ^ h >> shift) * mul & M32
    return h ^ h >> 16


def value(bits):
    """(v, e) of a double's bit pattern; zero is (0, 0). Subnormal, Inf and NaN are not the recipe's."""
    if not bits & M63:
        return 0, 0
    assert 0 < bits >> 52 & 0x7FF < 2047, hex(bits)
    sig = 1 << 52 | bits & M52
    return (-sig if bits >> 63 else sig), (bits >> 52 & 0x7FF) - 1075


def bits_of(v, e):
    """The bit pattern of v * 2**e, which must be a normal double with at most 53 significant bits."""
    mag = abs(v)
    top = mag.bit_length() - 1
    assert mag and top - (mag & -mag).bit_length() + 1 < 53 and 0 < 1023 + top + e < 2047, (v, e)
    return (v < 0) << 63 | (1023 + top + e) << 52 | (mag << 52 >> top if top <= 52 else mag >> top - 52) & M52


def band(nw, stage, base, rc, k, flip):
    h, lo = mix(nw, stage, base + (rc * 4 + k) * 2), mix(nw, stage, base + (rc * 4 + k) * 2 + 1)
    v = (h & 0x800FFFFF | 512 + (h >> 21 & 0x3FF) << 20) << 32 | (lo & 0xFC000000 if stage == 2 else lo)
    return v ^ (1 << 64) - 1 if flip else v


def onehot(nw, stage, rc, k):
    if rc + mix(nw, stage, IDX_ROT) & 3 != k:
        return 0
    h = mix(nw, stage, IDX_HOT + rc * 2)
    if stage != 2:
        return (h & 0x80000000 | 513 + (h & 0xFFFF) % 1022 << 20) << 32
    return (h & 0x800FFFFF | 513 + (h >> 20 & 0x7FF) % 1021 << 20) << 32 | mix(nw, stage, IDX_HOT + rc * 2 + 1) & 0xF8000000


def exponent_field(nw, stage, base, rc):
    return 535 + mix(nw, stage, base + rc) % 977


def operand(side, stage, t, rc, k, nw):
    """A[rc][k] (side 0) or B[rc][k] (side 1) of pass / tile t, as a bit pattern."""
    base = (IDX_A, IDX_B)[side]
    if stage in SUM_STAGES:                    # odd 27-bit (A) or 20-bit (B) significand, the row's / column's exponent
        h, e = mix(nw, stage, base + (rc * 4 + k) * 2), exponent_field(nw, stage, (IDX_EA, IDX_EB)[side], rc)
        if side:
            return (h & 0x800FFFFC | 2 | e << 20) << 32
        return (h & 0x800FFFFF | e << 20) << 32 | (h << 6 & 0xF8000000) | 0x04000000
    return onehot(nw, stage, rc, k) if side == (stage != 1) else band(nw, stage, base, rc, k, t)


def quantum(stage, row, col, nw):              # the exponent of q of output (row, col) of a sum stage
    return exponent_field(nw, stage, IDX_EA, row) + exponent_field(nw, stage, IDX_EB, col) - 2046 - 45


def row_col(stage, d):    # row of A, column of B behind double d of a tile (4x4x4_4b: block b owns 4b..4b+3 of both)
    return (4 * (d >> 4) + (d >> 2 & 3), 4 * (d >> 4) + (d & 3)) if stage >= 5 else (d >> 4, d & 15)


def terms(stage, t, row, col, nw):
    """[C, p0..p3] of one output as (v, e), the neg bit of stage 4's tile t applied (1,0,0 / 0,1,0 / 0,0,1)."""
    out = [(0, 0)]
    if stage in SUM_STAGES:
        h, lo = mix(nw, stage, IDX_C + (row * 16 + col) * 2), mix(nw, stage, IDX_C + (row * 16 + col) * 2 + 1)
        ga = (h & 0x1FFFF) << 32 | lo | 1
        out = [(-ga if (h >> 31) ^ (stage == 4 and t == 2) else ga, quantum(stage, row, col, nw))]
    for k in range(4):
        (va, ea), (vb, eb) = value(operand(0, stage, t, row, k, nw)), value(operand(1, stage, t, col, k, nw))
        out.append((-va * vb if stage == 4 and t < 2 else va * vb, ea + eb))
    return out


def expected_tile(stage, t, nw):
    words = []
    for d in range(DOUBLES[stage]):
        ts = [(v, e) for v, e in terms(stage, t, *row_col(stage, d), nw) if v]
        low = min(e for _, e in ts)
        b = bits_of(sum(v << e - low for v, e in ts), low)
        words += [b & M32, b >> 32]
    return words


@functools.lru_cache(maxsize=None)
def tiles_image(nonce, grid):
    """tiles[wg][4992] as uint32: wave 0's twelve tiles of every workgroup. Computed once per (nonce, grid), read-only."""
    t = np.array([[w for s in range(STAGES) for p in range(TILES[s])
                   for w in expected_tile(s, p, wave_nonce(nonce, wg, 0))] for wg in range(grid)], dtype=np.uint32)
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
    keep = [REC_MAGIC, REC_WG, REC_NONCE, REC_WORDS - 1]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    return rec[:, REC_BAD:REC_BAD + STAGES], np.argwhere(tiles.reshape(grid, WG_WORDS) != want).tolist()
