"""Independent reference of the sparse (2:4) MFMA datapath check (mi355x_mfma_datapath_sparse): the operand recipe of
native/src/health/datapath_sparse_kernel.h and the image a correct kernel writes, in Python integers. An element is
(u, x), meaning the exact value u * 2**x. Nothing here goes through the header; tests/test_native_datapath_sparse.py
holds the two equal."""
import functools

import numpy as np

M32 = 0xFFFFFFFF
STAGES, WAVES, REC_WORDS = 10, 4, 32
F16, BF16, I8, FP8 = 0, 1, 2, 3                                   # data kinds; FP8: A e4m3, B e5m2
SEL_A, SEL_B, SUM = 0, 1, 2                                       # selection with A hot / B hot, sum
KIND = (F16, F16, F16, F16, F16, BF16, BF16, I8, I8, FP8)
DIM = (32, 32, 32, 32, 16, 32, 16, 32, 16, 32)
MODE = (SEL_A, SEL_B, SEL_A, SUM, SUM, SUM, SEL_A, SUM, SUM, SUM)
ABID = (0, 0, 1, 0, 0, 0, 0, 0, 0, 0)
STAGE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = tuple(sum(STAGE_WORDS[:s]) for s in range(STAGES))
WG_WORDS = sum(STAGE_WORDS)                    # 7936
MAGIC = int.from_bytes(b"DPSP", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8
IDX_A, IDX_B, IDX_C, IDX_HOT, IDX_ROT, IDX_E, IDX_PAIR = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800, (0x3900, 0x3A00), 0x3B00
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))          # the index pairs used: first < second
# (mantissa bits, x of the quantum at exponent field 0): a normal is (2**mb + m) * 2**(E + x0)
FLOATS = {"f16": (10, -25), "bf16": (7, -134), "e4m3": (3, -10), "e5m2": (2, -17)}
Q_BIAS = {F16: -45, BF16: -268, FP8: -27}                         # q = 2**(Ea + Eb + this)


def wave_nonce(nonce, wg, wave):
    return ((nonce ^ (wg * 0x9E3779B1 & M32)) + wave * 0x85EBCA77) & M32


def mix(nw, stage, idx):
    h = nw ^ ((stage + 0x83) * 0x9E3779B1 & M32) ^ (idx * 0x85EBCA77 & M32)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h = (h ^ h >> shift) * mul & M32
    return h ^ h >> 16


def groups(stage):
    return 64 // DIM[stage]


def bits(stage):
    return 8 if KIND[stage] in (I8, FP8) else 16


def kb(stage):
    """Dense K positions of a lane group: 16 (16-bit data) or 32."""
    return 256 // bits(stage)


def fmt(stage, side):
    return {F16: "f16", BF16: "bf16", I8: "i8", FP8: ("e4m3", "e5m2")[side]}[KIND[stage]]


def k_of(stage, h, p):
    """The dense k of position p (4 * group + index field) of lane group h of A: two runs of KB / 2 (measured on an
    MI355X). Element e of lane group h of B is k = KB * h + e."""
    n, r, m = kb(stage), kb(stage) // 2, groups(stage) // 2
    return n * (2 * (h % m) + p // r) + r * (h // m) + p % r


def pair(stage, row, h, t, nw):
    hp = mix(nw, stage, IDX_PAIR)
    if MODE[stage] == SEL_B:
        return (h * 4 + t + (hp & 7)) % 6
    return (row + (hp >> (h * 8 + t) % 29 & 7)) % 6


def index_fields(stage, row, h, nw):
    """The pairs of the groups of (row, lane group h): what the instruction reads."""
    return [PAIRS[pair(stage, row, h, t, nw)] for t in range(kb(stage) // 4)]


def _pack(pairs):
    return sum((a | b << 2) << 4 * t for t, (a, b) in enumerate(pairs))


def index_word(stage, row, h, nw):
    """The index register of lane (row, lane group h): 32 bits, or 16 in the half abid selects and another legal
    pattern in the other half."""
    w = _pack(index_fields(stage, row, h, nw))
    if bits(stage) == 8:
        return w
    step = 1 + (mix(nw, stage, IDX_PAIR) >> 29 & 3)
    other = _pack(PAIRS[(pair(stage, row, h, t, nw) + step) % 6] for t in range(4))
    return w << 16 | other if ABID[stage] else w | other << 16


def _band(stage, h):
    def f16(v):
        return v & 0x83FF | 1 + ((v >> 10 & 0x1F) * 30 >> 5) << 10

    def bf16(v):
        return v & 0x807F | 97 + ((v >> 7 & 0xFF) * 62 >> 8) << 7
    one = {F16: f16, BF16: bf16}.get(KIND[stage])
    return one(h & 0xFFFF) | one(h >> 16) << 16 if one else h


def _hot(stage, rc, nw):
    h = mix(nw, stage, IDX_HOT + rc)
    return h >> 31 << 15 | (37 + (h & 0xFFFF) % 181 << 7 if KIND[stage] == BF16 else 1 + (h & 0xFFFF) % 30 << 10)


def hot_slot(stage, rc, nw):
    return (rc + (mix(nw, stage, IDX_ROT) & 31)) % (groups(stage) * 8)


def exp_field(stage, side, rc, nw):
    h = mix(nw, stage, IDX_E[side] + rc)
    return 97 + h % 62 if KIND[stage] == BF16 else 1 + h % (14 if fmt(stage, side) == "e4m3" else 30)


def _odd(stage, side, h, e):
    f = fmt(stage, side)
    if f == "f16":
        narrow = (side == 0) == (stage == 4)
        return (h & 0x83E083E0 | 0x00200020 if narrow else h & 0x83FF83FF | 0x00010001) | e << 10 | e << 26
    if f == "bf16":
        return h & 0x807F807F | 0x00010001 | e << 7 | e << 23
    return h & 0x83838383 | 0x01010101 | e * 0x04040404 if f == "e5m2" else h & 0x87878787 | 0x01010101 | e * 0x08080808


def hot_k(stage, col, nw):
    """Stage 1: the dense k of column col's hot element, the one slot (col + rot) mod 16 of A selects."""
    slot = hot_slot(stage, col, nw)
    ha, c = slot >> 3, slot & 7
    return k_of(stage, ha, 4 * (c >> 1) + index_fields(stage, 0, ha, nw)[c >> 1][c & 1])


def fragment(stage, side, rc, h, nw):
    """The dwords of the fragment of (row / column rc, lane group h): 4 of compressed A (side 0), 8 of dense B (1)."""
    n, base = (4, 8)[side], (IDX_A, IDX_B)[side] + (rc * 4 + h) * (4, 8)[side]
    hot = MODE[stage] == (SEL_A, SEL_B)[side]
    if hot:
        at = hot_slot(stage, rc, nw) - h * 8 if side == 0 else hot_k(stage, rc, nw) - h * 16
        return [_hot(stage, rc, nw) << 16 * (at & 1) if at >> 1 == d else 0 for d in range(n)]
    if MODE[stage] != SUM or KIND[stage] == I8:
        even = [_band(stage, mix(nw, stage, base + (d & ~1))) for d in range(n)]
        return [w ^ M32 if d & 1 else w for d, w in enumerate(even)]
    return [_odd(stage, side, mix(nw, stage, base + d), exp_field(stage, side, rc, nw)) for d in range(n)]


def value(code, f):
    """(u, x) of an element's code."""
    if f == "i8":
        return code - 256 * (code >> 7), 0
    mb, x0 = FLOATS[f]
    width = 8 if f[0] == "e" else 16
    field, m = code >> mb & (1 << width - 1 - mb) - 1, code & (1 << mb) - 1
    if not field:
        assert m == 0, (code, f)                                  # the recipe holds no subnormal
        return 0, 0
    u = 1 << mb | m
    return (-u if code >> width - 1 else u), field + x0


def elements(stage, side, rc, h, nw):
    w = bits(stage)
    stream = sum(d << 32 * i for i, d in enumerate(fragment(stage, side, rc, h, nw)))
    return [value(stream >> w * e & (1 << w) - 1, fmt(stage, side)) for e in range((128, 256)[side] // w)]


def c_term(stage, row, col, nw):
    """C[row][col] as (ga, x): ga * 2**x; (0, 0) in the selection stages."""
    if MODE[stage] != SUM:
        return 0, 0
    h = mix(nw, stage, IDX_C + row * 32 + col)
    if KIND[stage] == I8:
        return (h >> 1) - (h >> 31 << 31), 0
    ga = h & 0xFFFFF | 1
    return (-ga if h >> 31 else ga), exp_field(stage, 0, row, nw) + exp_field(stage, 1, col, nw) + Q_BIAS[KIND[stage]]


def f32_bits(v, x):
    """The bit pattern of v * 2**x, which must be a normal f32 with at most 24 significant bits."""
    mag = abs(v)
    top = mag.bit_length() - 1
    assert mag and top - (mag & -mag).bit_length() + 1 < 24 and 0 < 127 + top + x < 255, (v, x)
    return (v < 0) << 31 | 127 + top + x << 23 | (mag << 23 >> top if top <= 23 else mag >> top - 23) & 0x7FFFFF


def dense_a(stage, nw):
    """[row][k] -> (u, x): the compressed A expanded through the index; the unselected positions are (0, 0)."""
    out = [[(0, 0)] * (groups(stage) * kb(stage)) for _ in range(DIM[stage])]
    for row in range(DIM[stage]):
        for h in range(groups(stage)):
            fields = index_fields(stage, row, h, nw)
            for c, v in enumerate(elements(stage, 0, row, h, nw)):
                out[row][k_of(stage, h, 4 * (c >> 1) + fields[c >> 1][c & 1])] = v
    return out


def dense_b(stage, nw):
    """[col][k] -> (u, x)."""
    return [[v for h in range(groups(stage)) for v in elements(stage, 1, col, h, nw)] for col in range(DIM[stage])]


def expected_tile(stage, nw):
    a, b, words = dense_a(stage, nw), dense_b(stage, nw), []
    for row in range(DIM[stage]):
        for col in range(DIM[stage]):
            ts = [t for t in [c_term(stage, row, col, nw)] + [(ua * ub, xa + xb) for (ua, xa), (ub, xb) in
                                                               zip(a[row], b[col])] if t[0]]
            if KIND[stage] == I8:
                words.append(sum(v for v, _ in ts) & M32)
                continue
            low = min(x for _, x in ts)
            words.append(f32_bits(sum(v << x - low for v, x in ts), low))
    return words


@functools.lru_cache(maxsize=None)
def _wg_tiles(nw):
    return tuple(w for s in range(STAGES) for w in expected_tile(s, nw))


@functools.lru_cache(maxsize=None)
def tiles_image(nonce, grid):
    """tiles[wg][7936] as uint32: wave 0's ten tiles of every workgroup. Computed once per (nonce, grid), read-only."""
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
    assert not rec[:, REC_BAD + STAGES:].any(), rec.tolist()
    return rec[:, REC_BAD:REC_BAD + STAGES], np.argwhere(tiles.reshape(grid, WG_WORDS) != want).tolist()
