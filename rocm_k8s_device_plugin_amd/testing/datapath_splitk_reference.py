"""Independent reference of the split-K GEMM check (mi355x_splitk_fill, mi355x_mfma_datapath_splitk,
mi355x_splitk_drain): the image a correct run leaves -- per-workgroup records, the D tiles after every split's partial
was added, the per-tile ledgers -- in integers, on the operands of datapath_gemm_reference at ksteps_total =
splits * ksteps. Nothing here goes through the headers; tests/test_native_datapath_splitk.py holds the two equal."""
import functools

import numpy as np

from . import datapath_gemm_reference as dg

M32 = dg.M32
TILE, KSTEP, SPLITS, KSTEPS, CUS_PER_TILE = dg.TILE, dg.KSTEP, 8, 4, 8
TILE_WORDS, LEDGER_WORDS, REC_WORDS, WAVES, STAGES = TILE * TILE, 8, 32, 4, 4
MAGIC = int.from_bytes(b"DPSK", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_TILES, REC_SPLITS, REC_KSTEPS, REC_FOLD = 0, 1, 2, 3, 4, 8, 9, 10, 16
LED_ARRIVALS, LED_WHO, LED_A_SUM, LED_A_XOR, LED_B_SUM, LED_B_XOR = range(6)


def k_range(split, ksteps):
    return slice(split * ksteps * KSTEP, (split + 1) * ksteps * KSTEP)


def partial(nonce, tile, splits, ksteps, split):
    """What one workgroup adds: the integers (in quanta) of A_t[:, range] . B[range, :]."""
    a, b, ks = dg.a_elements(nonce, tile, splits * ksteps), dg.b_elements(nonce, splits * ksteps), k_range(split, ksteps)
    au = dg.units(a[:, ks], dg.exp_fields(dg.wg_seed(nonce, tile), dg.SPACE_EA)[:, None])
    return au @ dg.units(b[ks], dg.exp_fields(nonce, dg.SPACE_EB)[None, :])


def integers(nonce, tile, splits, ksteps, skip=()):
    """n[128][128]: D_t in quanta after C and the partials of every split not in `skip`."""
    return dg.ga(nonce, tile) + sum(partial(nonce, tile, splits, ksteps, s) for s in range(splits) if s not in skip)


def folds(nonce, tile, splits, ksteps, split):
    """The 16 fold words of a record: wave v reads rows 64*(v>>1).. of A and columns 64*(v&1).. of B, its k-range."""
    a, b, ks = dg.a_elements(nonce, tile, splits * ksteps), dg.b_elements(nonce, splits * ksteps), k_range(split, ksteps)
    out = []
    for v in range(WAVES):
        out += [*dg.fold(a[64 * (v >> 1):64 * (v >> 1) + 64, ks]), *dg.fold(b[ks, 64 * (v & 1):64 * (v & 1) + 64])]
    return out


def fold_slot(stage, word):
    """Where word `word` (wave * 2 + {xor, sum}) of feed stage `stage` sits in a record."""
    return REC_FOLD + (word >> 1) * 4 + stage * 2 + (word & 1)


def ledger(nonce, tile, splits, ksteps, skip=()):
    """The tile's 8 ledger words after the workgroups of every split not in `skip`: arrivals, xor of nonce ^ wg, sum
    and xor over the 16-bit elements of the parts of A_t and of B they read, two zero words."""
    a, b = dg.a_elements(nonce, tile, splits * ksteps), dg.b_elements(nonce, splits * ksteps)
    led = [0] * LEDGER_WORDS
    for s in (s for s in range(splits) if s not in skip):
        (ax, asum), (bx, bsum) = dg.fold(a[:, k_range(s, ksteps)]), dg.fold(b[k_range(s, ksteps)])
        led[LED_ARRIVALS] += 1
        led[LED_WHO] ^= nonce ^ (tile * splits + s)
        led[LED_A_SUM], led[LED_A_XOR] = (led[LED_A_SUM] + asum) & M32, led[LED_A_XOR] ^ ax
        led[LED_B_SUM], led[LED_B_XOR] = (led[LED_B_SUM] + bsum) & M32, led[LED_B_XOR] ^ bx
    return led


@functools.lru_cache(maxsize=None)
def _healthy(tiles, splits, ksteps, nonce):
    recs = np.zeros((tiles * splits, REC_WORDS), dtype=np.uint32)
    d = np.zeros((tiles, TILE_WORDS), dtype=np.uint32)
    led = np.zeros((tiles, LEDGER_WORDS), dtype=np.uint32)
    for t in range(tiles):
        d[t] = dg.f32_words(integers(nonce, t, splits, ksteps), dg.qx(nonce, t)).reshape(-1)
        led[t] = ledger(nonce, t, splits, ksteps)
        for s in range(splits):
            wg = t * splits + s
            recs[wg, :3] = (MAGIC, wg, nonce ^ wg)
            recs[wg, REC_TILES:REC_KSTEPS + 1] = (tiles, splits, ksteps)
            recs[wg, REC_FOLD:] = folds(nonce, t, splits, ksteps, s)
    for x in (recs, d, led):
        x.setflags(write=False)
    return recs, d, led


def healthy(tiles, splits, ksteps, nonce):
    """(records, D tiles, ledgers) of a correct run; where it ran (XCC id, HW_ID words) is left zero."""
    return tuple(x.copy() for x in _healthy(tiles, splits, ksteps, nonce))


def image_bytes(records, d, ledgers) -> bytes:
    return b"".join(np.ascontiguousarray(x, dtype="<u4").tobytes() for x in (records, d, ledgers))


def compare_raw(records, d, ledgers, tiles, splits, ksteps, nonce, want=None):
    """What a launch left against the image (or `want`): the (row, word) lists of fold words, D words and ledger words
    that differ. Identity, placement and the zero words of the records are asserted."""
    want_rec, want_d, want_led = want or healthy(tiles, splits, ksteps, nonce)
    rec = records.reshape(tiles * splits, REC_WORDS)
    keep = [REC_MAGIC, REC_WG, REC_NONCE, REC_TILES, REC_SPLITS, REC_KSTEPS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, rec[:, keep].tolist())
    assert (rec[:, REC_XCC] < 16).all() and (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec.tolist()
    assert not rec[:, REC_KSTEPS + 1:REC_FOLD].any(), rec.tolist()
    return (np.argwhere(rec[:, REC_FOLD:] != want_rec[:, REC_FOLD:]).tolist(),
            np.argwhere(d.reshape(tiles, TILE_WORDS) != want_d).tolist(),
            np.argwhere(ledgers.reshape(tiles, LEDGER_WORDS) != want_led).tolist())


def acc_word(wave, lane, index):
    """The D word (row * 128 + column) that accumulator word `index` ((row block * 4 + column block) * 4 + register) of
    lane `lane` of wave `wave` is added to: v_mfma_f32_16x16x32_bf16 leaves D[4*(l>>4) + r][l&15] in register r."""
    row = 64 * (wave >> 1) + 16 * (index >> 4) + 4 * (lane >> 4) + (index & 3)
    return row * TILE + 64 * (wave & 1) + 16 * (index >> 2 & 3) + (lane & 15)
