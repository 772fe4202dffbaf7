"""Independent reference of the fused attention check (mi355x_attn_fill, mi355x_mfma_datapath_attn): the operands and
their bytes, S by full 64-term dot products, m, l and O as integers in quanta and as f32 words, the per-wave folds, and
a replay of the online recurrence that asserts the quantum and bound argument of datapath_attn_kernel.h at every step.
Numpy integers throughout; nothing here goes through the headers; tests/test_native_datapath_attn.py holds the two
equal."""
import functools

import numpy as np

from .datapath_gemm_reference import M32, fold, mix, wg_seed

D, QBLOCK, KBLOCK, QBLOCKS, KBLOCKS, KBLOCKS_MAX, CUS_PER_HEAD = 64, 128, 64, 4, 4, 8, 4
ML_WORDS, O_WORDS, REC_WORDS, WAVES, STAGES = QBLOCK * 2, QBLOCK * D, 32, 4, 4
MAGIC = int.from_bytes(b"DPAT", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_HEADS, REC_QBLOCKS, REC_KBLOCKS, REC_EXP_INEXACT, REC_FOLD = \
    0, 1, 2, 3, 4, 8, 9, 10, 11, 16
SPACE_SHAPE, SPACE_Q, SPACE_K, SPACE_LIVE, SPACE_V, SPACE_EV, SPACE_X = range(0x50, 0x57)
M_START = -1024


def _idx(rows, cols=32):
    r, c = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(cols, dtype=np.uint64), indexing="ij")
    return r * cols + c


def _signed(h, mag):
    return np.where(h >> 31 & 1, -mag, mag).astype(np.int64)


def shapes(nonce):
    """The 32 pairs' shapes: 0 = Q (a, a), K (x, -x); 1 = Q (a, 2a), K (2x, -x)."""
    return (mix(nonce, SPACE_SHAPE, np.arange(32, dtype=np.uint64)) & 1).astype(np.int64)


def a_values(nonce, head, qblocks):
    """a[query][pair] = +-{1,2}."""
    h = mix(wg_seed(nonce, head), SPACE_Q, _idx(qblocks * QBLOCK)).astype(np.int64)
    return _signed(h, 1 + (h & 1))


def live(nonce, head, kblocks):
    """(pairs[key][3], t[key][3]): the three distinct live pairs of every key and their t = +-1."""
    h = mix(wg_seed(nonce, head), SPACE_LIVE, np.arange(kblocks * KBLOCK, dtype=np.uint64)).astype(np.int64)
    p0 = h & 31
    p1 = p0 + 1 + (h >> 5 & 15) & 31
    p2 = p1 + 1 + (h >> 9 & 7) & 31
    pairs = np.stack([p0, p1, p2], axis=1)
    assert all(len(set(row)) == 3 for row in pairs.tolist())
    return pairs, np.stack([np.where(h >> 12 + i & 1, -1, 1) for i in range(3)], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def q_integers(nonce, head, qblocks):
    """Q[query][64] as integers."""
    a, sh = a_values(nonce, head, qblocks), shapes(nonce)
    out = np.stack([a, a * (1 + sh)[None, :]], axis=2).reshape(-1, D)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def k_integers(nonce, head, kblocks):
    """K[key][64] as integers: the first element of a live pair carries t."""
    h = mix(wg_seed(nonce, head), SPACE_K, _idx(kblocks * KBLOCK)).astype(np.int64)
    x, sh = _signed(h, 2 + (h & 0xFFFF) % 5), shapes(nonce)
    first = x * (1 + sh)[None, :]
    pairs, t = live(nonce, head, kblocks)
    np.add.at(first, (np.arange(len(pairs))[:, None], pairs), t)
    out = np.stack([first, -x], axis=2).reshape(-1, D)
    out.setflags(write=False)
    return out


def ev(nonce, head):
    """The exponent fields of V's 64 columns, 101..158."""
    return (101 + mix(wg_seed(nonce, head), SPACE_EV, np.arange(D, dtype=np.uint64)) % 58).astype(np.int64)


@functools.lru_cache(maxsize=None)
def v_integers(nonce, head, kblocks):
    """V[key][64] in units of 2**(Ev_d - 127): +-{1,2,3}."""
    h = mix(wg_seed(nonce, head), SPACE_V, _idx(kblocks * KBLOCK)).astype(np.int64)
    h16 = np.stack([h & 0xFFFF, h >> 16], axis=2).reshape(-1, D)
    out = np.where(h16 >> 15, -1, 1) * (1 + (h16 & 0x7FFF) % 3)
    out.setflags(write=False)
    return out


def bf16_ints(n, exp_field=127):
    """The bf16 bit patterns of the non-zero integers n times 2**(exp_field - 127)."""
    mag = np.abs(n)
    assert (mag > 0).all() and (mag < 256).all()
    top = np.floor(np.log2(mag)).astype(np.int64)
    return (n < 0).astype(np.int64) << 15 | exp_field + top << 7 | (mag << 7 - top) & 0x7F


def operand_bytes(heads, qblocks, kblocks, nonce):
    """What mi355x_attn_fill writes: (Q, K, V) as bytes, all heads."""
    def cat(rows):
        return b"".join(r.astype("<u2").tobytes() for r in rows)
    return (cat(bf16_ints(q_integers(nonce, h, qblocks)) for h in range(heads)),
            cat(bf16_ints(k_integers(nonce, h, kblocks)) for h in range(heads)),
            cat(bf16_ints(v_integers(nonce, h, kblocks), ev(nonce, h)[None, :]) for h in range(heads)))


def scores(nonce, head, qblocks, kblocks):
    """S[query][key] by the full 64-term dot products."""
    return q_integers(nonce, head, qblocks) @ k_integers(nonce, head, kblocks).T


def live_scores(nonce, head, qblocks, kblocks):
    """S[query][key] from the three live terms alone: what dpat_score computes."""
    a, (pairs, t) = a_values(nonce, head, qblocks), live(nonce, head, kblocks)
    return (a[:, pairs] * t[None, :, :]).sum(axis=2)


def state(s, v):
    """(m, l in quanta of 2**-12, O in quanta of 2**(Ev_d - 139)) of the scores s[query][key] and V's integers."""
    m = s.max(axis=1)
    p = np.int64(1) << (s - m[:, None] + 12)
    return m, p.sum(axis=1), p @ v


def online(s, v, flips=()):
    """The recurrence block by block, as the kernel runs it, asserting at every step that S - m stays in -12..0, that
    the rescale keeps l and O whole numbers of quanta and that all magnitudes stay below 2**24. Returns
    (m, l, O, rises): rises[query] lists the blocks after the first in which the query's running max rose."""
    nq, nk = s.shape
    m = np.full(nq, M_START, dtype=np.int64)
    l, o, labs, oabs = (np.zeros(shape, dtype=np.int64) for shape in (nq, (nq, D), nq, (nq, D)))
    rises = [[] for _ in range(nq)]
    for b in range(nk // KBLOCK):
        sb, vb = s[:, b * KBLOCK:(b + 1) * KBLOCK], v[b * KBLOCK:(b + 1) * KBLOCK]
        m_new = np.maximum(m, sb.max(axis=1))
        k = m - m_new                                                   # <= 0: the ldexp's integer
        if b:
            assert (k >= -12).all()
            for i in np.flatnonzero(k).tolist():
                rises[i].append(b)
            assert (l % (1 << -k) == 0).all() and (o % (np.int64(1) << -k)[:, None] == 0).all()   # still whole quanta
            l, o, labs, oabs = l >> -k, o >> (-k)[:, None], labs >> -k, oabs >> (-k)[:, None]
        assert (sb - m_new[:, None] <= 0).all() and (sb - m_new[:, None] >= -12).all()
        assert (s[:, :(b + 1) * KBLOCK].min(axis=1) - m_new >= -12).all()  # over the whole row so far
        p = np.int64(1) << (sb - m_new[:, None] + 12)
        l, o, labs, oabs = l + p.sum(axis=1), o + p @ vb, labs + p.sum(axis=1), oabs + p @ np.abs(vb)
        assert labs.max() < 1 << 24 and oabs.max() < 1 << 24            # every partial sum fits an f32 significand
        m = m_new
    return m, l, o, rises


def f32_words(n, x):
    """The bit patterns of n * 2**x, |n| < 2**24; zero is +0."""
    n, x = np.broadcast_arrays(np.asarray(n, dtype=np.int64), np.asarray(x, dtype=np.int64))
    mag = np.abs(n)
    assert (mag < 1 << 24).all()
    top = np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64)
    words = (n < 0).astype(np.int64) << 31 | 127 + top + x << 23 | (mag << 23 - top) & 0x7FFFFF
    return np.where(mag == 0, 0, words).astype(np.uint32)


def words(nonce, head, m, l, o):
    """(m / l words [query][2], O words [query][64]) of a head's integers."""
    ml = np.stack([f32_words(m, 0), f32_words(l, -12)], axis=1)
    return ml, f32_words(o, (ev(nonce, head) - 139)[None, :])


def folds(nonce, head, kblocks):
    """The 16 fold words of a record: every wave reads the head's whole K and V."""
    k, v = bf16_ints(k_integers(nonce, head, kblocks)), bf16_ints(v_integers(nonce, head, kblocks), ev(nonce, head)[None, :])
    return [*fold(k), *fold(v)] * WAVES


def fold_slot(stage, word):
    """Where word `word` (wave * 2 + {xor, sum}) of feed stage `stage` sits in a record."""
    return REC_FOLD + (word >> 1) * 4 + stage * 2 + (word & 1)


def image_of(nonce, heads, qblocks, kblocks, head_scores):
    """(records, m / l words, O words) of the run whose S is head_scores(head)."""
    grid = heads * qblocks
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    ml = np.zeros((grid, ML_WORDS), dtype=np.uint32)
    o = np.zeros((grid, O_WORDS), dtype=np.uint32)
    for head in range(heads):
        w_ml, w_o = words(nonce, head, *state(head_scores(head), v_integers(nonce, head, kblocks)))
        for qb in range(qblocks):
            wg = head * qblocks + qb
            recs[wg, :3] = (MAGIC, wg, nonce ^ wg)
            recs[wg, REC_HEADS:REC_KBLOCKS + 1] = (heads, qblocks, kblocks)
            recs[wg, REC_FOLD:] = folds(nonce, head, kblocks)
            ml[wg] = w_ml[qb * QBLOCK:(qb + 1) * QBLOCK].reshape(-1)
            o[wg] = w_o[qb * QBLOCK:(qb + 1) * QBLOCK].reshape(-1)
    return recs, ml, o


@functools.lru_cache(maxsize=None)
def _healthy(heads, qblocks, kblocks, nonce):
    out = image_of(nonce, heads, qblocks, kblocks, lambda head: scores(nonce, head, qblocks, kblocks))
    for x in out:
        x.setflags(write=False)
    return out


def healthy(heads, qblocks, kblocks, nonce):
    """(records, m / l words, O words) of a correct run; where it ran (XCC id, HW_ID) and exp_inexact are left zero."""
    return tuple(x.copy() for x in _healthy(heads, qblocks, kblocks, nonce))


def image_bytes(records, ml, o) -> bytes:
    return b"".join(np.ascontiguousarray(x, dtype="<u4").tobytes() for x in (records, ml, o))


def compare_raw(records, ml, o, heads, qblocks, kblocks, nonce, want=None):
    """What a launch left against the image (or `want`): the (workgroup, word) lists of fold words, m / l words and O
    words that differ. Identity, placement and the zero words of the records are asserted; exp_inexact is not judged."""
    grid = heads * qblocks
    want_rec, want_ml, want_o = want or healthy(heads, qblocks, kblocks, nonce)
    rec = records.reshape(grid, REC_WORDS)
    keep = [REC_MAGIC, REC_WG, REC_NONCE, REC_HEADS, REC_QBLOCKS, REC_KBLOCKS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    assert not rec[:, REC_EXP_INEXACT + 1:REC_FOLD].any(), rec.tolist()
    return (np.argwhere(rec[:, REC_FOLD:] != want_rec[:, REC_FOLD:]).tolist(),
            np.argwhere(ml.reshape(grid, ML_WORDS) != want_ml).tolist(),
            np.argwhere(o.reshape(grid, O_WORDS) != want_o).tolist())


def s_word(wave, lane, index):
    """(query of the workgroup, key of the head) of S accumulator word `index` (block * 32 + sub-block * 16 + register)
    of lane `lane` of wave `wave`: register r of a 32x32 block is row (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)."""
    r = index & 15
    return 32 * wave + (lane & 31), (index >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


def o_word(wave, lane, index):
    """The O word (query * 64 + d) of O accumulator word `index` (d-half * 16 + register) of that lane."""
    r = index & 15
    return (32 * wave + (lane & 31)) * D + 32 * (index >> 4) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
