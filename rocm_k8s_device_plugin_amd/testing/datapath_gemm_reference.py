"""Independent reference of the bf16 GEMM pipeline check (mi355x_gemm_fill, mi355x_mfma_datapath_gemm): the operand
recipe of native/src/health/datapath_gemm_kernel.h, the D image and the per-wave folds a correct kernel writes, in
integers (numpy int64 holds every sum: all magnitudes of an output stay below 2**24 quanta). Nothing here goes through
the header; tests/test_native_datapath_gemm.py holds the two equal."""
import functools

import numpy as np

M32 = 0xFFFFFFFF
TILE, KSTEP, KSTEPS, KSTEPS_MAX = 128, 64, 16, 32
WG_WORDS, REC_WORDS, WAVES, STAGES = TILE * TILE, 32, 4, 3
MAGIC = int.from_bytes(b"DPGM", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_KSTEPS, REC_FOLD = 0, 1, 2, 3, 4, 8, 16
SPACE_A, SPACE_B, SPACE_C, SPACE_EA, SPACE_EB, SPACE_X = 0x40, 0x41, 0x42, 0x43, 0x44, 0x45
E_BAND = range(101, 159)                       # exponent fields of rows of A and columns of B
LDS_TILE_BYTES = 16384


def wg_seed(nonce, wg):
    return (nonce ^ (wg * 0x9E3779B1 & M32)) & M32


def mix(seed, space, idx):
    """The hash, on Python integers or on uint64 arrays of indices."""
    h = seed ^ ((space + 0x21) * 0x9E3779B1 & M32) ^ (idx * 0x85EBCA77 & M32)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h = (h ^ h >> shift) * mul & M32
    return h ^ h >> 16


def exp_fields(seed, space):
    """The 128 exponent fields of the rows of A (SPACE_EA, a workgroup's seed) or the columns of B (SPACE_EB, the nonce)."""
    return E_BAND.start + mix(seed, space, np.arange(TILE, dtype=np.uint64)) % len(E_BAND)


def _pairs(h, e, full):
    """Two bf16 of one hash word: full +-(128+m), m odd, field e; narrow +-(8+m'), m' odd, field e-4, low bits zero."""
    wide = h & 0x807F807F | 0x00010001 | e << 7 | e << 23
    narrow = h & 0x80708070 | 0x00100010 | e - 4 << 7 | e - 4 << 23
    return np.where(full, wide, narrow)


@functools.lru_cache(maxsize=None)
def a_elements(nonce, wg, ksteps):
    """A_wg[128][K] as bf16 bit patterns (uint16 in int64)."""
    K, seed = ksteps * KSTEP, wg_seed(nonce, wg)
    row, kk = np.meshgrid(np.arange(TILE, dtype=np.uint64), np.arange(K // 2, dtype=np.uint64), indexing="ij")
    w = _pairs(mix(seed, SPACE_A, row * (K // 2) + kk), exp_fields(seed, SPACE_EA)[:, None], (kk >> 4 & 1) == 0)
    out = np.stack([w & 0xFFFF, w >> 16], axis=2).reshape(TILE, K).astype(np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def b_elements(nonce, ksteps):
    """B[K][128] as bf16 bit patterns: one panel for all workgroups."""
    K = ksteps * KSTEP
    k, cc = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(TILE // 2, dtype=np.uint64), indexing="ij")
    h = mix(nonce, SPACE_B, k * 64 + cc)
    e = exp_fields(nonce, SPACE_EB).reshape(TILE // 2, 2)
    full = (k >> 5 & 1) == 1
    lo = _pairs(h, e[None, :, 0], full) & 0xFFFF
    hi = _pairs(h, e[None, :, 1], full) >> 16
    out = np.stack([lo, hi], axis=2).reshape(K, TILE).astype(np.int64)
    out.setflags(write=False)
    return out


def units(elements, fields):
    """The elements as signed integers in quanta of 2**(E-134), E broadcast against them."""
    mag = (128 + (elements & 0x7F)) >> (fields.astype(np.int64) - (elements >> 7 & 0xFF))
    return np.where(elements >> 15 & 1, -mag, mag)


def ga(nonce, wg):
    """C's integers: ga[128][128], odd, below 2**20 in magnitude."""
    h = mix(wg_seed(nonce, wg), SPACE_C, np.arange(WG_WORDS, dtype=np.uint64)).reshape(TILE, TILE).astype(np.int64)
    mag = h & 0xFFFFF | 1
    return np.where(h >> 31, -mag, mag)


def qx(nonce, wg):
    """log2 of the quantum of every output."""
    ea, eb = exp_fields(wg_seed(nonce, wg), SPACE_EA), exp_fields(nonce, SPACE_EB)
    return ea.astype(np.int64)[:, None] + eb.astype(np.int64)[None, :] - 268


def integers(nonce, wg, ksteps, a=None, b=None):
    """n[128][128]: D in quanta. `a` / `b` replace the operands' bit patterns (fault models)."""
    a = a_elements(nonce, wg, ksteps) if a is None else a
    b = b_elements(nonce, ksteps) if b is None else b
    au = units(a, exp_fields(wg_seed(nonce, wg), SPACE_EA)[:, None])
    bu = units(b, exp_fields(nonce, SPACE_EB)[None, :])
    return ga(nonce, wg) + au @ bu


def f32_words(n, x):
    """The bit patterns of n * 2**x: n non-zero, below 2**24 in magnitude."""
    mag = np.abs(n)
    assert (mag > 0).all() and (mag < 1 << 24).all()
    top = np.floor(np.log2(mag)).astype(np.int64)          # exact below 2**53
    assert (127 + top + x > 0).all() and (127 + top + x < 255).all()
    return ((n < 0).astype(np.int64) << 31 | 127 + top + x << 23 | (mag << 23 - top) & 0x7FFFFF).astype(np.uint32)


def fold(elements):
    """(xor, sum modulo 2**32) over 16-bit elements."""
    return int(np.bitwise_xor.reduce(elements, axis=None)), int(elements.sum()) & M32


def folds(nonce, wg, ksteps, a=None, b=None):
    """The 16 fold words of a record: wave v reads rows 64*(v>>1).. of A and columns 64*(v&1).. of B, all K."""
    a = a_elements(nonce, wg, ksteps) if a is None else a
    b = b_elements(nonce, ksteps) if b is None else b
    out = []
    for v in range(WAVES):
        out += [*fold(a[64 * (v >> 1):64 * (v >> 1) + 64]), *fold(b[:, 64 * (v & 1):64 * (v & 1) + 64])]
    return out


def fold_slot(stage, word):
    """Where word `word` (wave * 2 + {xor, sum}) of feed stage `stage` sits in a record."""
    return REC_FOLD + (word >> 1) * 4 + stage * 2 + (word & 1)


@functools.lru_cache(maxsize=None)
def _healthy(grid, nonce, ksteps):
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    tiles = np.zeros((grid, WG_WORDS), dtype=np.uint32)
    for wg in range(grid):
        recs[wg, :3] = (MAGIC, wg, nonce ^ wg)
        recs[wg, REC_KSTEPS] = ksteps
        recs[wg, REC_FOLD:REC_FOLD + 16] = folds(nonce, wg, ksteps)
        tiles[wg] = f32_words(integers(nonce, wg, ksteps), qx(nonce, wg)).reshape(-1)
    recs.setflags(write=False)
    tiles.setflags(write=False)
    return recs, tiles


def healthy(grid, nonce, ksteps):
    """(records, tiles) of a correct run; where it ran (XCC id, HW_ID words) is left zero."""
    recs, tiles = _healthy(grid, nonce, ksteps)
    return recs.copy(), tiles.copy()


def image_bytes(records, tiles) -> bytes:
    return np.ascontiguousarray(records, dtype="<u4").tobytes() + np.ascontiguousarray(tiles, dtype="<u4").tobytes()


def operand_bytes(grid, nonce, ksteps) -> bytes:
    """What mi355x_gemm_fill writes: the A panels, then B."""
    return b"".join(a_elements(nonce, wg, ksteps).astype("<u2").tobytes() for wg in range(grid)) + \
        b_elements(nonce, ksteps).astype("<u2").tobytes()


def projection_ok(n_row, nonce, wg, ksteps, row) -> bool:
    """The verdict's step 2 on one row of integers: both projections equal the operands'."""
    b = units(b_elements(nonce, ksteps), exp_fields(nonce, SPACE_EB)[None, :])
    a = units(a_elements(nonce, wg, ksteps), exp_fields(wg_seed(nonce, wg), SPACE_EA)[:, None])[row]
    xs = (np.ones(TILE, dtype=np.int64), (mix(nonce, SPACE_X, np.arange(TILE, dtype=np.uint64)) & 0xFF | 1).astype(np.int64))
    return all(int(n_row @ x) == int(ga(nonce, wg)[row] @ x) + int(a @ (b @ x)) for x in xs)


def lds_source(dword):
    """Which operand dword lands at dword `dword` (0..8191) of a step's LDS buffer: ("a", row, k) or ("b", k, col) of
    its first element, k within the step. Chunks of 16 bytes are swizzled: A position p of row r holds k-chunk
    p ^ ((r >> 1) & 7), B position p of row k holds column chunk p ^ ((k & 3) << 2)."""
    byte = dword * 4
    if byte < LDS_TILE_BYTES:
        row, p = byte // 128, byte % 128 // 16
        return "a", row, (p ^ (row >> 1 & 7)) * 8 + byte % 16 // 2
    byte -= LDS_TILE_BYTES
    k, p = byte // 256, byte % 256 // 16
    return "b", k, (p ^ ((k & 3) << 2)) * 8 + byte % 16 // 2


def wrong_kernel_models(nonce, ksteps):
    """name -> D integers of workgroup 0 under a kernel fault that a correct image must differ from."""
    a, b = a_elements(nonce, 0, ksteps), b_elements(nonce, ksteps)
    K = ksteps * KSTEP
    steps = [slice(s * KSTEP, (s + 1) * KSTEP) for s in range(ksteps)]

    def with_steps(order):
        """The k-steps of both operands taken in `order` (a list of step numbers, any length)."""
        aa = np.concatenate([a[:, steps[s]] for s in order], axis=1)
        bb = np.concatenate([b[steps[s]] for s in order], axis=0)
        au = units(aa, exp_fields(wg_seed(nonce, 0), SPACE_EA)[:, None])
        return ga(nonce, 0) + au @ units(bb, exp_fields(nonce, SPACE_EB)[None, :])

    untransposed = b.copy()
    for s in steps:                                             # each 64 x 128 step tile read as [n][k] in 64 x 64 halves
        for half in (slice(0, 64), slice(64, 128)):
            untransposed[s, half] = b[s, half].T
    # the A tile of step s paired with the B tile of step s ^ 1: the buffers of one operand swapped
    swapped_b = np.concatenate([b[steps[s ^ 1 if (s ^ 1) < ksteps else s]] for s in range(ksteps)], axis=0)
    halves = a.reshape(TILE, K // 2, 2)[:, :, ::-1].reshape(TILE, K)
    return {"B read untransposed": integers(nonce, 0, ksteps, b=untransposed),
            "LDS buffers swapped": integers(nonce, 0, ksteps, b=swapped_b),
            "one k-step dropped": with_steps(list(range(ksteps - 1))),
            "one k-step repeated": with_steps(list(range(ksteps)) + [0]),
            "halves swapped within a dword": integers(nonce, 0, ksteps, a=halves)}


def compare_raw(records, tiles, nonce, grid, ksteps):
    """What a launch left: ((wg, record word) of the fold words, (wg, D word) of the tile words that differ from the
    image). Identity, placement and the zero words of the records are asserted."""
    rec, (want_rec, want) = records.reshape(grid, REC_WORDS), healthy(grid, nonce, ksteps)
    keep = [REC_MAGIC, REC_WG, REC_NONCE, REC_KSTEPS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    assert not rec[:, REC_KSTEPS + 1:REC_FOLD].any(), rec.tolist()
    fold_diff = np.argwhere(rec[:, REC_FOLD:] != want_rec[:, REC_FOLD:])
    return [(int(w), int(i) + REC_FOLD) for w, i in fold_diff], np.argwhere(tiles.reshape(grid, WG_WORDS) != want).tolist()
