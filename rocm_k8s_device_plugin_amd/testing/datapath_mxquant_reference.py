"""Independent reference of the MX quantise check (mi355x_mxquant_fill, mi355x_mfma_datapath_mxquant): the operand
recipe of native/src/health/datapath_mxquant_kernel.h, the OCP MX quantisation rule on f32 words in integers, the
quantised image, Y and the per-wave folds a correct kernel writes, the wrong-kernel models, and `check`, which asserts
the recipe's properties. Nothing here goes through the headers; tests/test_native_datapath_mxquant.py holds the two equal."""
import functools

import numpy as np

from .datapath_mxgemm_reference import E2M1_UNITS, M32, fold, mix, wg_seed

TILE, HSTEPS, HSTEPS_MAX = 128, 4, 4
WG_WORDS, REC_WORDS, WAVES, STAGES = TILE * TILE, 32, 4, 4
MAGIC = int.from_bytes(b"DPMQ", "big")
REC_XCC, REC_HWID, REC_FOLD = 3, 4, 8
(SPACE_SHAPE, SPACE_A, SPACE_ROW, SPACE_WX, SPACE_LIVE, SPACE_BLK, SPACE_W2, SPACE_SB, SPACE_DB,
 SPACE_C) = range(0x70, 0x7A)
MID4 = (1, 3, 5, 7, 10, 14, 20)                # the e2m1 grid's midpoints in quarters: code c | c + 1
GRID4 = (0, 2, 4, 6, 8, 12, 16, 24)            # the grid in quarters
FIX = 38                                       # a scaled magnitude is held in units of 2**-(FIX + 2)
GUARD = 8                                      # Y integers carry 8 fraction bits, so that a faulty scale may be lower
CLASSES = ("exact", "down", "up", "tie_down_even", "tie_up_even", "tie_subnormal", "quarter_to_zero", "saturated")


def img_words(hsteps):
    return 2176 * hsteps


def _u64(n):
    return np.arange(n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def rows(nonce, wg):
    """(high row [128], g_i [128], a [128][64]) of X_wg."""
    seed = wg_seed(nonce, wg)
    rh = mix(seed, SPACE_ROW, _u64(TILE)).astype(np.int64)
    tok, pair = np.meshgrid(_u64(TILE), _u64(64), indexing="ij")
    h = mix(seed, SPACE_A, tok * 64 + pair).astype(np.int64)
    mag = np.where(pair < 32, 1 + 2 * (h & 1), 1 + (h & 0xFFFF) % 3)
    mag = np.where((rh & 1)[:, None] == 1, mag, 1)
    return rh & 1, (rh >> 8) % 49 - 24, np.where(h >> 31, -mag, mag)


@functools.lru_cache(maxsize=None)
def hidden(nonce, hsteps):
    """Per hidden column: (p0, p1, t0, t1) [N]; per block: (class, f_b) [N / 32]."""
    n = _u64(TILE * hsteps)
    blk = _u64(4 * hsteps)
    cls = (mix(nonce, SPACE_BLK, blk) % 3).astype(np.int64)
    f = ((blk ^ np.uint64(mix(nonce, SPACE_BLK, 0xFFFF))) & 1).astype(np.int64)
    h = mix(nonce, SPACE_LIVE, n).astype(np.int64)
    c = np.repeat(cls, 32)
    m0 = 1 + 2 * ((h >> 10 & 0xFF) % (c + 1))
    m1 = 2 * (1 + np.where(c == 2, h >> 18 & 1, 0))
    return (h & 31, 32 + (h >> 5 & 31), np.where(h >> 20 & 1, -m0, m0), np.where(h >> 21 & 1, -m1, m1)), (cls, f)


def shapes(nonce):
    return (mix(nonce, SPACE_SHAPE, _u64(64)) & 1).astype(np.int64)


def s_integers(nonce, wg, hsteps):
    """S [128][N] from the live terms alone: H = S * 2**(g_i + f_b)."""
    (p0, p1, t0, t1), _ = hidden(nonce, hsteps)
    a = rows(nonce, wg)[2]
    return a[:, p0] * t0 + a[:, p1] * t1


def bf16(n, x):
    """The bf16 bit patterns of n * 2**x, n non-zero integers below 256 in magnitude."""
    mag = np.abs(n)
    assert (mag > 0).all() and (mag < 256).all()
    top = np.floor(np.log2(mag)).astype(np.int64)
    return (n < 0).astype(np.int64) << 15 | 127 + top + x << 7 | (mag << 7 - top) & 0x7F


def x_elements(nonce, wg):
    """X_wg [128][128] as bf16 bit patterns: the pair (a, a) or (a, 2a), times 2**g_i."""
    _, g, a = rows(nonce, wg)
    return np.stack([bf16(a, g[:, None]), bf16(np.where(shapes(nonce), 2 * a, a), g[:, None])], axis=2).reshape(TILE, TILE)


@functools.lru_cache(maxsize=None)
def w1_integers(nonce, hsteps):
    """W1 [N][128] as integers w, W1 = w * 2**f_b: the pair (x, -x) or (2x, -x), the live pairs' first element + t."""
    (p0, p1, t0, t1), _ = hidden(nonce, hsteps)
    n, pair = np.meshgrid(_u64(TILE * hsteps), _u64(64), indexing="ij")
    h = mix(nonce, SPACE_WX, n * 64 + pair).astype(np.int64)
    x = np.where(h >> 31, -1, 1) * (6 + (h & 0xFFFF) % 5)
    first = np.where(shapes(nonce), 2 * x, x)
    idx = np.arange(TILE * hsteps)
    first[idx, p0] += t0
    first[idx, p1] += t1
    return np.stack([first, -x], axis=2).reshape(TILE * hsteps, TILE)


def w1_elements(nonce, hsteps):
    return bf16(w1_integers(nonce, hsteps), np.repeat(hidden(nonce, hsteps)[1][1], 32)[:, None])


@functools.lru_cache(maxsize=None)
def w2_codes(nonce, hsteps):
    """The e2m1 codes [column][N] of W2: free codes, never +-0."""
    col, kd = np.meshgrid(_u64(TILE), _u64(16 * hsteps), indexing="ij")
    nib = (mix(nonce, SPACE_W2, col * (16 * hsteps) + kd)[:, :, None] >> (4 * _u64(8))) & 0xF
    return np.where(nib & 7 == 0, nib | 1, nib).reshape(TILE, TILE * hsteps).astype(np.int64)


def sb_base(nonce):
    return 112 + (mix(nonce, SPACE_SB, _u64(TILE)) % 31).astype(np.int64)


@functools.lru_cache(maxsize=None)
def sb_bytes(nonce, hsteps):
    col, blk = np.meshgrid(_u64(TILE), _u64(4 * hsteps), indexing="ij")
    return sb_base(nonce)[:, None] + (mix(nonce, SPACE_DB, col * 64 + blk) >> 13 & 1).astype(np.int64)


def ga(nonce, wg):
    h = mix(wg_seed(nonce, wg), SPACE_C, _u64(WG_WORDS)).reshape(TILE, TILE).astype(np.int64)
    mag = h & 0xFFFFF | 1
    return np.where(h >> 31, -mag, mag)


def f32_words(n, x):
    """The bit patterns of n * 2**x (0 is +0): every n must fit a 24-bit significand, the result a normal f32."""
    mag = np.abs(n)
    top = np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64)          # exact below 2**53
    sig = np.where(top >= 23, mag >> np.maximum(top - 23, 0), mag << np.maximum(23 - top, 0))
    assert (np.where(top >= 23, sig << np.maximum(top - 23, 0), sig >> np.maximum(23 - top, 0)) == mag).all()
    assert ((127 + top + x > 0) & (127 + top + x < 255) | (mag == 0)).all()
    return np.where(mag == 0, 0, (n < 0).astype(np.int64) << 31 | 127 + top + x << 23 | sig & 0x7FFFFF).astype(np.uint32)


def h_words(nonce, wg, hsteps):
    """The f32 words of H [128][N], from S."""
    return f32_words(s_integers(nonce, wg, hsteps), rows(nonce, wg)[1][:, None] + np.repeat(hidden(nonce, hsteps)[1][1], 32)[None, :])


def quantise(words, ties="even", saturate=True, scale="exponent", amax="abs", times=1, counts=None):
    """(codes [r][N], E [r][N / 32]) of f32 words [r][N] by the OCP MX rule in integers: E = max(ef, 3) - 2 with ef
    the exponent field of the block's amax, each element round_to_nearest_even(h * 2**-(E-127)) on the e2m1 grid,
    saturated. The keywords are the wrong-kernel models; `counts` (a dict) receives how many elements took each case
    of the rule."""
    w = words.astype(np.int64)
    mag, neg = w & 0x7FFFFFFF, w >> 31 & 1
    blk = mag.reshape(w.shape[0], -1, 32)
    if amax == "half":                                      # one half-wave's 16 columns of the block only
        am = blk[:, :, (np.arange(32) >> 2 & 1) == 0].max(axis=2)
    elif amax == "signed":
        am = np.where(neg, 0, mag).reshape(blk.shape).max(axis=2)
    else:
        am = blk.max(axis=2)
    if amax == "neighbour":
        am = np.roll(am, 1, axis=1)
    ef = (am >> 23) + ((am & 0x7FFFFF) != 0 if scale == "ceil" else 0)
    e8 = np.maximum(ef, 3) - 2
    e, m = mag >> 23, np.where(mag >> 23 > 0, mag & 0x7FFFFF | 0x800000, 0)
    k = np.clip(e - 150 - times * (np.repeat(e8, 32, axis=1) - 127) + FIX + 2, -30, 22)
    fixed = np.where(k >= 0, m << np.maximum(k, 0), m >> np.maximum(-k, 0) | (m & (1 << np.maximum(-k, 0)) - 1 != 0))
    if ties == "truncate":
        code = sum((fixed >= g << FIX).astype(np.int64) for g in GRID4[1:])
    else:
        code = sum((fixed > mp << FIX) | (fixed == mp << FIX) & bool(c & 1 or ties == "away") for c, mp in enumerate(MID4))
    if not saturate:                                        # what rounds to 8 has no code: the magnitude wraps
        code = np.where(fixed >= 28 << FIX, 0, code)
    if counts is not None:
        grid = np.array(GRID4)[code] << FIX
        sat, tie = fixed > 24 << FIX, sum(fixed == mp << FIX for mp in MID4).astype(bool)
        found = {"exact": fixed == grid, "down": (fixed > grid) & ~tie & ~sat, "up": (fixed < grid) & ~tie,
                 "tie_down_even": tie & (fixed > grid), "tie_up_even": tie & (fixed < grid),
                 "tie_subnormal": (fixed == 1 << FIX) | (fixed == 3 << FIX), "quarter_to_zero": fixed == 1 << FIX,
                 "saturated": sat}
        counts.update({name: counts.get(name, 0) + int(found[name].sum()) for name in CLASSES})
    return code | neg << 3, e8


def pack(c):
    """Codes [..][N] as dwords [..][N / 8]: element n in bits 4 * (n & 1).. of byte n / 2."""
    return np.ascontiguousarray(c[..., 0::2] | c[..., 1::2] << 4, dtype=np.uint8).view("<u4").astype(np.int64)


def gathered(raw):
    """The two scale VGPRs (lane group 0, 1) made of a slab's four bytes [..][4]: bytes (h, 2 + h, h, 2 + h)."""
    two = raw[..., 0:2] | raw[..., 2:4] << 8
    return two | two << 16


def y_integers(nonce, wg, hsteps, codes, e8, sb=None):
    """Y [128][128] in units of 2**-GUARD quanta, q = 2**(g_i + SB_j - 132): ga + 2 sum uq uw 2**(E - 125 - g_i + d').
    Asserts the header's bound: the magnitudes of C and of all products sum to less than 2**24 quanta."""
    g = rows(nonce, wg)[1]
    sb = sb_bytes(nonce, hsteps) if sb is None else sb
    up = np.repeat(e8 - 125 - g[:, None], 32, axis=1) + GUARD
    assert (up >= 0).all()
    uq = np.where(codes >> 3, -1, 1) * E2M1_UNITS[codes & 7] << up
    w2 = w2_codes(nonce, hsteps)
    uw = np.where(w2 >> 3, -1, 1) * E2M1_UNITS[w2 & 7] << np.repeat(sb - sb_base(nonce)[:, None], 32, axis=1)
    c = ga(nonce, wg) << GUARD
    assert (np.abs(c) + 2 * np.abs(uq) @ np.abs(uw).T < 1 << 24 + GUARD).all()
    return c + 2 * uq @ uw.T


def y_words(nonce, wg, hsteps, codes, e8, sb=None):
    qx = rows(nonce, wg)[1][:, None] + sb_base(nonce)[None, :] - 132
    return f32_words(y_integers(nonce, wg, hsteps, codes, e8, sb), qx - GUARD).reshape(-1)


def image_of(codes, e8):
    """The quantised image of one workgroup: 128 rows of code dwords, then 128 rows of scale dwords (a byte a block)."""
    return np.concatenate([pack(codes).reshape(-1), np.ascontiguousarray(e8, dtype=np.uint8).view("<u4").astype(np.int64).reshape(-1)]).astype(np.uint32)


def record(nonce, wg, hsteps, e8):
    """The record: where it ran (XCC id, HW_ID words) is left zero. Every wave reads all of W1, W2 of its column half,
    the activations' scales of its row half and W2's of its column half."""
    rec = np.zeros(REC_WORDS, dtype=np.uint32)
    rec[:4] = (MAGIC, wg, nonce ^ wg, hsteps << 8)
    w1 = w1_elements(nonce, hsteps)
    w1d = w1[:, 0::2] | w1[:, 1::2] << 16
    w2d = pack(w2_codes(nonce, hsteps))
    sa, sw = gathered(e8.reshape(TILE, hsteps, 4)), gathered(sb_bytes(nonce, hsteps).reshape(TILE, hsteps, 4))
    for v in range(WAVES):
        r, c = slice(64 * (v >> 1), 64 * (v >> 1) + 64), slice(64 * (v & 1), 64 * (v & 1) + 64)
        rec[REC_FOLD + 6 * v:REC_FOLD + 6 * v + 6] = [*fold(w1d), *fold(w2d[c]), *fold(np.concatenate([sa[r], sw[c]]))]
    return rec


def fold_slot(stage, word):
    """Where fold word `word` of feed stage `stage` sits in a record: stage 0 word = wave * 2 + {xor, sum} (W1), stage 1
    word = wave * 4 + {W2 xor, W2 sum, scale xor, scale sum}."""
    return REC_FOLD + (word >> 1) * 6 + (word & 1) if stage == 0 else REC_FOLD + (word >> 2) * 6 + 2 + (word & 3)


def image(nonce, wg, hsteps, hwords=None, **model):
    """(record, quantised image, Y tile) of workgroup wg, from H words (the recipe's unless given) under a model."""
    codes, e8 = quantise(h_words(nonce, wg, hsteps) if hwords is None else hwords, **model)
    return record(nonce, wg, hsteps, e8), image_of(codes, e8), y_words(nonce, wg, hsteps, codes, e8)


@functools.lru_cache(maxsize=None)
def _healthy(grid, nonce, hsteps):
    parts = tuple(np.stack(x) for x in zip(*(image(nonce, wg, hsteps) for wg in range(grid))))
    for p in parts:
        p.setflags(write=False)
    return parts


def healthy(grid, nonce, hsteps):
    """(records, images, tiles) of a correct run."""
    return tuple(p.copy() for p in _healthy(grid, nonce, hsteps))


def image_bytes(records, images, tiles) -> bytes:
    return b"".join(np.ascontiguousarray(p, dtype="<u4").tobytes() for p in (records, images, tiles))


def operand_bytes(grid, nonce, hsteps) -> bytes:
    """What mi355x_mxquant_fill writes: the X panels, W1, W2, W2's scale bytes."""
    return b"".join([x_elements(nonce, wg).astype("<u2").tobytes() for wg in range(grid)] +
                    [w1_elements(nonce, hsteps).astype("<u2").tobytes(), pack(w2_codes(nonce, hsteps)).astype("<u4").tobytes(),
                     sb_bytes(nonce, hsteps).astype(np.uint8).tobytes()])


MODELS = {"ties_away": dict(ties="away"), "truncate": dict(ties="truncate"), "no_saturation": dict(saturate=False),
          "scale_ceil": dict(scale="ceil"), "scale_neighbour": dict(amax="neighbour"), "amax_half_wave": dict(amax="half"),
          "amax_signed": dict(amax="signed"), "scale_twice": dict(times=2)}


def wrong_images(nonce, wg, hsteps):
    """name -> quantised image of a wrong kernel: the models of `quantise`, swapped nibbles, and a stuck bit in H."""
    out = {name: image(nonce, wg, hsteps, **kw)[1] for name, kw in MODELS.items()}
    codes, e8 = quantise(h_words(nonce, wg, hsteps))
    out["nibbles_swapped"] = image_of(codes.reshape(TILE, -1, 2)[:, :, ::-1].reshape(codes.shape), e8)
    out["stuck_code_bit"], out["stuck_scale_bit"] = image_of(codes | 2, e8), image_of(codes, e8 | 1)
    out["stuck_h_bit"] =image(nonce, wg, hsteps, hwords=h_words(nonce, wg, hsteps) | 1 << 22)[1]
    return out


def check(grid, nonce, hsteps):
    """Asserts the recipe's properties at one shape (datapath_mxquant_kernel.h); returns the counts of the rule's cases
    and of the codes. The 2**24 bound of every Y word is asserted in y_integers, on the way to the healthy image."""
    counts, seen = {}, np.zeros(16, dtype=np.int64)
    (p0, p1, t0, t1), (cls, f) = hidden(nonce, hsteps)
    assert (p0 < 32).all() and (p1 >= 32).all() and (t0 % 2 != 0).all() and (t1 % 2 == 0).all() and (f[1:] != f[:-1]).all()
    w1 = w1_integers(nonce, hsteps)
    assert (w1 != 0).all() and (np.abs(w1) <= 25).all()
    for wg in range(grid):
        high, g, a = rows(nonce, wg)
        s = s_integers(nonce, wg, hsteps)
        # 1: H is exact and O(1): the full 128-deep product equals the two live terms; every partial sum is small
        x = np.stack([a, np.where(shapes(nonce), 2 * a, a)], axis=2).reshape(TILE, TILE)
        assert (x @ w1.T == s).all() and (np.abs(x) @ np.abs(w1).T < 1 << 15).all() and (np.abs(s) <= 27).all()
        # 2: no block is zero, the maxima spread over several binades, the scale bytes stay in the band and vary
        peak = np.abs(s).reshape(TILE, -1, 32).max(axis=2)
        codes, e8 = quantise(h_words(nonce, wg, hsteps), counts=counts)
        assert (peak >= 1).all() and len(np.unique(np.floor(np.log2(peak)))) >= 3
        assert (e8 == 125 + np.floor(np.log2(peak)).astype(np.int64) + g[:, None] + f[None, :]).all()
        assert (e8 >= 97).all() and (e8 <= 158).all() and (e8.max(axis=1) != e8.min(axis=1)).all()
        seen += np.bincount(codes.reshape(-1), minlength=16)
    healthy(grid, nonce, hsteps)                            # 4: asserts the bound of every Y word
    # 3: every case of the rule and every code but -0
    assert all(counts[c] > 0 for c in CLASSES) and (np.delete(seen, 8) > 0).all(), (counts, seen)
    return counts, seen


def _patch_scale_fold(rec, wave, old, new):
    rec[REC_FOLD + 6 * wave + 4] ^= np.uint32(old ^ new)
    rec[REC_FOLD + 6 * wave + 5] = np.uint32((int(rec[REC_FOLD + 6 * wave + 5]) + new - old) & M32)


def injected(kind, nonce, wg, hsteps, inj):
    """(record, quantised image, Y tile) the inject build leaves for workgroup `wg` under one hook (the fields of
    raw_kernels' "inject")."""
    rec, img, tile = image(nonce, wg, hsteps)
    lane, v, index, mask = inj.get("lane", 0), inj.get("wave", 0), inj["index"], inj["mask"]
    if kind == "mfma":
        r, blk = index % 16, index // 16
        row = 64 * (v >> 1) + 32 * (blk >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        tile[row * TILE + 64 * (v & 1) + 32 * (blk & 1) + (lane & 31)] ^= mask
        return rec, img, tile
    if kind == "h":                                         # everything behind the accumulator follows
        r, hw = index % 16, h_words(nonce, wg, hsteps)
        hw[32 * v + (lane & 31), 32 * (index // 16) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)] ^= mask
        return image(nonce, wg, hsteps, hwords=hw)
    codes, e8 = quantise(h_words(nonce, wg, hsteps))
    if kind == "q":                                         # both waves of the row read it, and one stores it
        row, p, d = index // 16, index % 16 // 4, index % 4
        n0 = 128 * inj["step"] + 32 * (p ^ (row >> 2 & 3)) + 8 * d
        codes[row, n0:n0 + 8] ^= mask >> 4 * np.arange(8) & 0xF
        return rec, image_of(codes, e8), y_words(nonce, wg, hsteps, codes, e8)
    assert kind == "scale"                                  # one lane of one wave, from one sub-step of one slab on
    step, kk, t, h = index >> 3, index >> 2 & 1, index & 3, lane >> 5
    line = 64 * (v & 1 if t >= 2 else v >> 1) + 32 * (t & 1) + (lane & 31)
    used = sum(0xFF << 8 * (2 * (step & 1) + sub) for sub in range(kk, 2))
    assert mask & ~used == 0                                # only bytes the slab's remaining MFMAs select
    s = (sb_bytes(nonce, hsteps) if t >= 2 else e8).copy()
    old = int(gathered(s[line, 4 * step:4 * step + 4])[h])
    for sub in range(2):                                    # byte 2 * parity + sub of the VGPR is block 2 * sub + h
        s[line, 4 * step + 2 * sub + h] ^= mask >> 8 * (2 * (step & 1) + sub) & 0xFF
    _patch_scale_fold(rec, v, old, old ^ mask)
    bad = y_words(nonce, wg, hsteps, codes, *((e8, s) if t >= 2 else (s, None))).reshape(TILE, TILE)
    r, c = (slice(64 * (v >> 1), 64 * (v >> 1) + 64), slice(64 * (v & 1), 64 * (v & 1) + 64))
    tile.reshape(TILE, TILE)[r, c] = bad[r, c]
    return rec, img, tile


def compare_raw(records, images, tiles, want_rec, want_img, want_tiles):
    """What a launch left against an image: ((wg, record word) of the fold words, (wg, dword) of the image, (wg, word)
    of Y that differ). Identity and placement words of the records are asserted."""
    rec = records.reshape(want_rec.shape)
    assert (rec[:, :3] == want_rec[:, :3]).all() and (rec[:, REC_XCC] >> 8 == want_rec[:, REC_XCC] >> 8).all(), rec[:, :4]
    assert (rec[:, REC_XCC] & 0xFF < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    return ([(int(w), int(i) + REC_FOLD) for w, i in np.argwhere(rec[:, REC_FOLD:] != want_rec[:, REC_FOLD:])],
            np.argwhere(images.reshape(want_img.shape) != want_img).tolist(),
            np.argwhere(tiles.reshape(want_tiles.shape) != want_tiles).tolist())
