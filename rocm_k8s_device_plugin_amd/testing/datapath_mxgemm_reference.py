"""Independent reference of the MXFP4 GEMM pipeline check (mi355x_mxgemm_fill, mi355x_mfma_datapath_mxgemm): the
operand recipe of native/src/health/datapath_mxgemm_kernel.h, the D image and the per-wave folds a correct kernel
writes, in integers (numpy int64 holds every sum: all magnitudes of an output stay below 2**24 quanta, asserted).
Nothing here goes through the header; tests/test_native_datapath_mxgemm.py holds the two equal."""
import functools

import numpy as np

M32 = 0xFFFFFFFF
TILE, KSTEP, KSTEPS, KSTEPS_MAX = 128, 256, 8, 8
WG_WORDS, REC_WORDS, WAVES, STAGES = TILE * TILE, 32, 4, 4
MAGIC = int.from_bytes(b"DPMX", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_FOLD = 0, 1, 2, 3, 4, 8
SPACE_A, SPACE_B, SPACE_C, SPACE_SA, SPACE_SB, SPACE_DA, SPACE_DB = 0x60, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66
SBASE = range(112, 143)                        # SA_i and SB_j
DELTAS = (4, 2)                                # d in 0..3 for A, d' in 0..1 for B
E2M1_UNITS = np.array([0, 1, 2, 3, 4, 6, 8, 12], dtype=np.int64)   # the magnitudes in units of 2**-1: 0.5 .. 6
LDS_TILE_BYTES = 16384


def worst_case_quanta(ksteps):
    """The header's bound: every product at 12 * 12 units with the largest d + d', twice that in quanta, plus |ga|."""
    return 2 * ksteps * KSTEP * int(E2M1_UNITS[-1]) ** 2 * 2 ** (DELTAS[0] - 1 + DELTAS[1] - 1) + (1 << 20)


assert worst_case_quanta(KSTEPS_MAX) == 10_485_760 < 1 << 24 <= worst_case_quanta(2 * KSTEPS_MAX)


def wg_seed(nonce, wg):
    return (nonce ^ (wg * 0x9E3779B1 & M32)) & M32


def mix(seed, space, idx):
    """The hash, on Python integers or on uint64 arrays of indices."""
    h = seed ^ ((space + 0x21) * 0x9E3779B1 & M32) ^ (idx * 0x85EBCA77 & M32)
    for shift, mul in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h = (h ^ h >> shift) * mul & M32
    return h ^ h >> 16


def _seed(nonce, wg):
    """A's panels are seeded per workgroup, B (wg None) by the nonce."""
    return nonce if wg is None else wg_seed(nonce, wg)


@functools.lru_cache(maxsize=None)
def codes(nonce, wg, ksteps):
    """The e2m1 codes [128][K] of A_wg, or of B ([column][k]) with wg None: free codes, never +-0."""
    K = ksteps * KSTEP
    line, kd = np.meshgrid(np.arange(TILE, dtype=np.uint64), np.arange(K // 8, dtype=np.uint64), indexing="ij")
    h = mix(_seed(nonce, wg), SPACE_B if wg is None else SPACE_A, line * (K // 8) + kd)
    nib = (h[:, :, None] >> (4 * np.arange(8, dtype=np.uint64))) & 0xF
    nib = np.where(nib & 7 == 0, nib | 1, nib).reshape(TILE, K).astype(np.int64)
    nib.setflags(write=False)
    return nib


def scale_base(nonce, wg):
    return SBASE.start + (mix(_seed(nonce, wg), SPACE_SB if wg is None else SPACE_SA,
                              np.arange(TILE, dtype=np.uint64)) % len(SBASE)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def scales(nonce, wg, ksteps):
    """The E8M0 bytes [128][K/32]: the line's base plus d (A) or d' (B) per scale block."""
    line, g = np.meshgrid(np.arange(TILE, dtype=np.uint64), np.arange(ksteps * 8, dtype=np.uint64), indexing="ij")
    d = mix(_seed(nonce, wg), SPACE_DB if wg is None else SPACE_DA, line * 64 + g) >> 13 & (DELTAS[wg is None] - 1)
    out = scale_base(nonce, wg)[:, None] + d.astype(np.int64)
    out.setflags(write=False)
    return out


def pack(c):
    """Codes [..][K] as bytes [..][K/2]: element k in bits 4 * (k & 1).. of byte k / 2."""
    return (c[..., 0::2] | c[..., 1::2] << 4).astype(np.uint8)


def dwords(c):
    return pack(c).view("<u4").astype(np.int64)


def scaled_units(c, s, base):
    """Elements times 2**(scale - base) as signed integers, in units of 2**-2 (a faulty scale may be base - 1)."""
    mag = E2M1_UNITS[c & 7] << np.repeat(s - base[:, None] + 1, 32, axis=1)
    return np.where(c >> 3, -mag, mag)


def ga(nonce, wg):
    """C's integers: ga[128][128], odd, below 2**20 in magnitude."""
    h = mix(wg_seed(nonce, wg), SPACE_C, np.arange(WG_WORDS, dtype=np.uint64)).reshape(TILE, TILE).astype(np.int64)
    mag = h & 0xFFFFF | 1
    return np.where(h >> 31, -mag, mag)


def qx(nonce, wg):
    """log2 of the quantum of every output: q = U / 2, U = 2**-2 * 2**(SA_i + SB_j - 254)."""
    return scale_base(nonce, wg)[:, None] + scale_base(nonce, None)[None, :] - 257


def integers(nonce, wg, ksteps, a=None, b=None, sa=None, sb=None):
    """n[128][128]: D in quanta. The keyword arguments replace codes or scale bytes (fault models). Asserts the
    header's bound: the magnitudes of C and of all products sum to less than 2**24 quanta."""
    a = codes(nonce, wg, ksteps) if a is None else a
    b = codes(nonce, None, ksteps) if b is None else b
    sa = scales(nonce, wg, ksteps) if sa is None else sa
    sb = scales(nonce, None, ksteps) if sb is None else sb
    au, bu = scaled_units(a, sa, scale_base(nonce, wg)), scaled_units(b, sb, scale_base(nonce, None))
    c = ga(nonce, wg)
    assert (np.abs(c) + np.abs(au) @ np.abs(bu).T // 2 < 1 << 24).all()
    return c + au @ bu.T // 2                              # a product is 2 ua ub 2**(d+d') quanta: the division is exact


def f32_words(n, x):
    """The bit patterns of n * 2**x: n non-zero, below 2**24 in magnitude, the result a normal f32."""
    mag = np.abs(n)
    assert (mag > 0).all() and (mag < 1 << 24).all()
    top = np.floor(np.log2(mag)).astype(np.int64)          # exact below 2**53
    assert (127 + top + x > 0).all() and (127 + top + x < 255).all()
    return ((n < 0).astype(np.int64) << 31 | 127 + top + x << 23 | (mag << 23 - top) & 0x7FFFFF).astype(np.uint32)


def fold(words):
    """(xor, sum modulo 2**32) over dwords."""
    return int(np.bitwise_xor.reduce(words, axis=None)), int(words.sum()) & M32


def gathered(s):
    """The scale VGPRs fed for scale bytes [lines][K/32]: per step, lane group h holds bytes h, 2+h, 4+h, 6+h."""
    steps = s.reshape(s.shape[0], -1, 4, 2)                                      # [line][step][op_sel byte][h]
    return (steps << (8 * np.arange(4))[None, None, :, None]).sum(axis=2)        # [line][step][h]


def folds(nonce, wg, ksteps, a=None, b=None, sa=None, sb=None):
    """The 24 fold words of a record: wave v reads rows 64*(v>>1).. of A and sa, columns 64*(v&1).. of B and sb."""
    a = dwords(codes(nonce, wg, ksteps) if a is None else a)
    b = dwords(codes(nonce, None, ksteps) if b is None else b)
    sa = gathered(scales(nonce, wg, ksteps) if sa is None else sa)
    sb = gathered(scales(nonce, None, ksteps) if sb is None else sb)
    out = []
    for v in range(WAVES):
        r, c = slice(64 * (v >> 1), 64 * (v >> 1) + 64), slice(64 * (v & 1), 64 * (v & 1) + 64)
        out += [*fold(a[r]), *fold(b[c]), *fold(np.concatenate([sa[r], sb[c]]))]
    return out


def fold_slot(stage, word):
    """Where word `word` (wave * 2 + {xor, sum}) of feed stage `stage` (A, B, scales) sits in a record."""
    return REC_FOLD + (word >> 1) * 6 + stage * 2 + (word & 1)


def image(nonce, wg, ksteps, **faults):
    """(record, tile) of workgroup wg; where it ran (XCC id, HW_ID words) is left zero."""
    rec = np.zeros(REC_WORDS, dtype=np.uint32)
    rec[:4] = (MAGIC, wg, nonce ^ wg, ksteps << 8)
    rec[REC_FOLD:] = folds(nonce, wg, ksteps, **faults)
    return rec, f32_words(integers(nonce, wg, ksteps, **faults), qx(nonce, wg)).reshape(-1)


@functools.lru_cache(maxsize=None)
def _healthy(grid, nonce, ksteps):
    recs, tiles = (np.stack(x) for x in zip(*(image(nonce, wg, ksteps) for wg in range(grid))))
    recs.setflags(write=False)
    tiles.setflags(write=False)
    return recs, tiles


def healthy(grid, nonce, ksteps):
    """(records, tiles) of a correct run."""
    recs, tiles = _healthy(grid, nonce, ksteps)
    return recs.copy(), tiles.copy()


def image_bytes(records, tiles) -> bytes:
    return np.ascontiguousarray(records, dtype="<u4").tobytes() + np.ascontiguousarray(tiles, dtype="<u4").tobytes()


def operand_bytes(grid, nonce, ksteps) -> bytes:
    """What mi355x_mxgemm_fill writes: the A panels, B, the A scale panels, B's scales."""
    wgs = list(range(grid))
    return b"".join([pack(codes(nonce, wg, ksteps)).tobytes() for wg in wgs + [None]] +
                    [scales(nonce, wg, ksteps).astype(np.uint8).tobytes() for wg in wgs + [None]])


def lds_source(dword):
    """Which operand dword lands at dword `dword` (0..8191) of a step's LDS buffer: ("a" or "b", row / column, dword of
    the step's 32 of that line). 16-byte chunks are swizzled: position p of row r holds k-chunk p ^ ((r >> 1) & 7)."""
    which, byte = "ab"[dword * 4 // LDS_TILE_BYTES], dword * 4 % LDS_TILE_BYTES
    row, p = byte // 128, byte % 128 // 16
    return which, row, (p ^ (row >> 1 & 7)) * 4 + dword % 4


def flip_codes(c, dword, mask):
    """Codes with `mask` xor-ed into dword `dword` (flat, over [128][K/8]) of their packed form."""
    d = dwords(c).reshape(-1).copy()
    d[dword] ^= mask
    by = d.astype("<u4").view(np.uint8).reshape(TILE, -1).astype(np.int64)
    return np.stack([by & 0xF, by >> 4], axis=2).reshape(c.shape)


def injected(kind, nonce, wg, ksteps, inj):
    """(record, tile) the inject build leaves for workgroup `wg` under one hook (the fields of raw_kernels' "inject").
    Only the target's reads see an lds or scale fault: those waves' folds and their D words change."""
    rec, tile = image(nonce, wg, ksteps)
    K = ksteps * KSTEP
    if kind == "mfma":
        r, blk, lane, v = inj["index"] % 16, inj["index"] // 16, inj["lane"], inj["wave"]
        row = 64 * (v >> 1) + 32 * (blk >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        tile[row * TILE + 64 * (v & 1) + 32 * (blk & 1) + (lane & 31)] ^= inj["mask"]
        return rec, tile
    if kind == "hbm":                                       # every reader sees it
        return image(nonce, wg, ksteps, a=flip_codes(codes(nonce, wg, ksteps), inj["index"] // 4,
                                                     (inj["mask"] & 0xFF) << 8 * (inj["index"] % 4)))
    if kind == "lds":                                       # the two waves that read this row / column see it
        which, line, d = lds_source(inj["index"])
        bad = flip_codes(codes(nonce, wg if which == "a" else None, ksteps), line * (K // 8) + inj["step"] * 32 + d,
                         inj["mask"])
        frec, ftile = image(nonce, wg, ksteps, **{which: bad})
        waves = [v for v in range(WAVES) if (v >> 1 if which == "a" else v & 1) == line >> 6]
    else:                                                   # scale: one lane of one wave, from one sub-step on
        step, kk, t, lane, v = inj["index"] >> 4, inj["index"] >> 2 & 3, inj["index"] & 3, inj["lane"], inj["wave"]
        which = "sa" if t < 2 else "sb"
        line = 64 * (v & 1 if t >= 2 else v >> 1) + 32 * (t & 1) + (lane & 31)
        s = scales(nonce, wg if t < 2 else None, ksteps).copy()
        for sub in range(4):                                # byte `sub` of the VGPR is block 2 * sub + (lane >> 5)
            s[line, step * 8 + 2 * sub + (lane >> 5)] ^= inj["mask"] >> 8 * sub & 0xFF
        frec, ftile = image(nonce, wg, ksteps, **{which: s})
        assert inj["mask"] >> 8 * kk << 8 * kk == inj["mask"]   # no byte of an earlier sub-step: D saw them unharmed
        waves = [v]
    for w in waves:
        rec[REC_FOLD + 6 * w:REC_FOLD + 6 * w + 6] = frec[REC_FOLD + 6 * w:REC_FOLD + 6 * w + 6]
        r, c = 64 * (w >> 1), 64 * (w & 1)
        tile.reshape(TILE, TILE)[r:r + 64, c:c + 64] = ftile.reshape(TILE, TILE)[r:r + 64, c:c + 64]
    return rec, tile


def compare_raw(records, tiles, want_rec, want_tiles):
    """What a launch left against an image: ((wg, record word) of the fold words, (wg, D word) of the tile words that
    differ). Identity and placement words of the records are asserted."""
    rec = records.reshape(want_rec.shape)
    assert (rec[:, :3] == want_rec[:, :3]).all() and (rec[:, REC_XCC] >> 8 == want_rec[:, REC_XCC] >> 8).all(), rec[:, :4]
    assert (rec[:, REC_XCC] & 0xFF < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    fold_diff = np.argwhere(rec[:, REC_FOLD:] != want_rec[:, REC_FOLD:])
    return ([(int(w), int(i) + REC_FOLD) for w, i in fold_diff],
            np.argwhere(tiles.reshape(want_tiles.shape) != want_tiles).tolist())
