"""The host's verdicts on what the chip sweep and the throughput check wrote
(native/src/health/chip_verify.h) and the JSON the probe prints for them
(probe_json.h), CPU only, against the independent reference in
testing/kernel_reference.py: healthy records, then one wrong thing at a time.

A corpus of cases is built once and run once through
native/tests/kernel_contract_cli.cpp (sweep-verdict / perf-verdict). A case is
a set of arrays plus variants: word replacements applied to it for one more
verdict each (testing/contract_cli.py). Every line must equal the reference:
integers and booleans exactly, printed doubles within half a unit of their
last digit plus 1e-9 relative. Each variant also names what it must show.
The same corpus then goes through the program built with
-fsanitize=address,undefined, whose output must be the same bytes."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing.contract_cli import COUNTERS, RECORDS, TILES

M32 = ref.M32
NONCE, ITERS, GRID = 0xDEADBEEF, 4, 256
WGS = (0, 1, 37, 255)
CLEAN = [0, 0, M32, M32]
GIB = 1 << 30

SWEEP_ZERO_KEYS = {"ordinal": 0, "hsa_error": 0, "cu_count": 0, "kernel_us": 0, "total_us": 0, "in_flight_s": 0,
                   "kept_queue": False}
PERF_ZERO_KEYS = {"ordinal": 0, "hsa_error": 0, "cu_count": 0, "total_us": 0, "in_flight_s": 0, "kept_queue": False}

# the probe's format strings before the JSON was built without a fixed buffer (and before a check's
# reply named its agent): the expectation of test_json_line_is_byte_identical_to_the_fixed_buffer_format,
# not used by the product
OLD_SWEEP_FORMAT = ("{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"iters\":%d,\"grid\":%d,"
                    "\"cu_count\":%d,\"num_xcc\":%d,\"records_ok\":%d,\"mfma_bad\":%u,\"lds_bad\":%u,"
                    "\"tile_bad\":%u,\"cus_covered\":%d,\"xccs_covered\":%d,\"all_resident\":%s,"
                    "\"wgs_per_xcc\":%s,\"kernel_us\":%.2f,\"arrival_spread_us\":%.2f,\"total_us\":%.1f,"
                    "\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}")
OLD_PERF_FORMAT = ("{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"bytes\":%llu,\"cu_count\":%d,"
                   "\"num_xcc\":%d,\"fill_us\":%.1f,\"check_us\":%.1f,\"check2_us\":%.1f,\"hbm_write_gbps\":%.1f,"
                   "\"hbm_read_gbps\":%.1f,\"hbm_bad_words\":%llu,\"hbm_bad_words_pass2\":%llu,\"hbm_first_bad\":%lld,\"mfma_iters\":%d,\"mfma_grid\":%d,"
                   "\"mfma_records_ok\":%d,\"mfma_checksum_mismatch\":%d,\"mfma_xccs\":%d,\"mfma_us\":%.1f,"
                   "\"mfma_tflops\":%.1f,\"clock_mhz_min\":%.0f,\"clock_mhz_median\":%.0f,\"clock_mhz_max\":%.0f,"
                   "\"xcd_clock_mhz\":%s,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}")


class Case:
    """One case of the corpus. variants: [(label, [(array, index, value)], expectations)];
    the case as given is variant "base"."""

    def __init__(self, kind, arrays, params, base_expect, variants=()):
        self.kind, self.params = kind, params
        self.first, self.second = arrays            # sweep: records, tiles; perf: records, counters
        self.variants = [("base", [], base_expect)] + list(variants)

    def blob(self):
        patches = [p for _, p, _ in self.variants[1:]]
        if self.kind == "sweep":
            return contract_cli.sweep_case(self.first, self.second, variants=patches, **self.params)
        return contract_cli.perf_case(self.first, self.second, variants=patches, **self.params)

    def words(self):
        """The two arrays as flat uint32 views a patch indexes."""
        return self.first.reshape(-1), self.second.reshape(-1).view(np.uint32)

    def reference(self):
        if self.kind == "sweep":
            return ref.sweep_verdict(self.first, self.second, **self.params)
        return ref.perf_verdict(self.first, self.second, **self.params)


def rec_word(wg, word):
    return wg * 16 + word


# ---- the corpus ------------------------------------------------------------------------------
def _record_variants(nonce, grid, wgs, gone):
    """What makes a sweep record absent or faulty, at each workgroup of `wgs`.
    `gone`: what every variant with one record absent must show."""
    out = []
    for w in wgs:
        out.append((f"magic@{w}", [(RECORDS, rec_word(w, ref.REC_MAGIC), ref.SWEEP_MAGIC ^ 1)], gone))
        out.append((f"wg_off_by_one@{w}", [(RECORDS, rec_word(w, ref.REC_WG), w + 1)], gone))
        if (nonce + w) & M32 != nonce ^ w:
            out.append((f"nonce_sum@{w}", [(RECORDS, rec_word(w, ref.REC_NONCE), (nonce + w) & M32)], gone))
        out.append((f"zero_record@{w}", [(RECORDS, rec_word(w, k), 0) for k in range(16)], gone))
        out.append((f"absent_with_mfma_bad@{w}", [(RECORDS, rec_word(w, ref.REC_MAGIC), 0),
                                                   (RECORDS, rec_word(w, ref.REC_MFMA_BAD), M32)],
                    dict(gone, mfma_bad=0)))
        faulty = {"ok": False, "records_ok": grid - 1, "cus_covered": grid, "all_resident": False}
        out.append((f"mfma_bad@{w}", [(RECORDS, rec_word(w, ref.REC_MFMA_BAD), 1)],
                    dict(faulty, mfma_bad=1, lds_bad=0, tile_bad=0)))
        out.append((f"lds_bad@{w}", [(RECORDS, rec_word(w, ref.REC_LDS_BAD), 1)],
                    dict(faulty, mfma_bad=0, lds_bad=1, tile_bad=0)))
    return out


def _tile_variants(tiles, grid, wgs):
    bits = tiles.reshape(grid, 1024).view(np.uint32)
    one = {"ok": False, "records_ok": grid - 1, "tile_bad": 1, "mfma_bad": 0, "cus_covered": grid}
    out = []
    for w in wgs:
        out += [(f"tile{w}[0]^bit{b}", [(TILES, w * 1024, int(bits[w, 0]) ^ 1 << b)], one) for b in range(32)]
        zeros = np.flatnonzero(bits[w] == 0)
        assert zeros.size, f"tile {w} holds no +0.0"
        out.append((f"negative_zero@{w}", [(TILES, w * 1024 + int(zeros[-1]), 0x80000000)], one))
        o = (w + 1) % grid
        differ = int((bits[w] != bits[o]).sum())
        assert differ > 512
        out.append((f"tiles_exchanged@{w}",
                    [(TILES, w * 1024 + e, int(bits[o, e])) for e in range(1024)]
                    + [(TILES, o * 1024 + e, int(bits[w, e])) for e in range(1024)],
                    {"ok": False, "records_ok": grid - 2, "tile_bad": 2 * differ}))
        out.append((f"tile_at_prefill@{w}", [(TILES, w * 1024 + e, M32) for e in range(1024)],
                    {"ok": False, "records_ok": grid - 1, "tile_bad": 1024}))
    return out


def _tile_bit_variants(tiles, grid, wgs):
    """Bit 0 and bit 31 of every element of the tile, at each workgroup of `wgs`."""
    bits = tiles.reshape(grid, 1024).view(np.uint32)
    one = {"ok": False, "records_ok": grid - 1, "tile_bad": 1}
    return [(f"tile{w}[{e}]^bit{b}", [(TILES, w * 1024 + e, int(bits[w, e]) ^ 1 << b)], one)
            for w in wgs for e in range(1024) for b in (0, 31)]


def _sweep_cases():
    cases = {}
    def healthy(grid, xcds):
        return {"ok": True, "records_ok": grid, "cus_covered": grid, "xccs_covered": xcds, "all_resident": True,
                "mfma_bad": 0, "lds_bad": 0, "tile_bad": 0}

    params = dict(grid=GRID, nonce=NONCE, iters=ITERS, num_xcc=8)
    recs, tiles = ref.healthy_sweep(GRID, NONCE, ITERS, ref.spread_placement(GRID, 8))
    gone = {"ok": False, "records_ok": GRID - 1, "cus_covered": GRID - 1, "xccs_covered": 8, "all_resident": False,
            "mfma_bad": 0, "lds_bad": 0, "tile_bad": 0}
    cases["sweep256"] = Case("sweep", (recs, tiles), params, dict(healthy(GRID, 8), wgs_per_xcc=[32] * 8),
                             _record_variants(NONCE, GRID, WGS, gone) + _tile_variants(tiles, GRID, WGS))
    for w in WGS:
        cases[f"sweep256_tile{w}_bits"] = Case("sweep", (recs.copy(), tiles.copy()), params, healthy(GRID, 8),
                                               _tile_bit_variants(tiles, GRID, (w,)))
    r, t = ref.healthy_sweep(32, 12345, 4, ref.spread_placement(32, 1))
    cases["sweep32_one_xcd"] = Case("sweep", (r, t), dict(grid=32, nonce=12345, iters=4, num_xcc=1),
                                    dict(healthy(32, 1), wgs_per_xcc=[32]))
    r, t = ref.healthy_sweep(4, 7, 4, ref.spread_placement(4, 2))
    cases["sweep4_no_xcd_count"] = Case("sweep", (r, t), dict(grid=4, nonce=7, iters=4, num_xcc=0),
                                        dict(healthy(4, 2), wgs_per_xcc=[2, 2, 0, 0, 0, 0, 0, 0]))
    for nonce in (0, 0xDEADBEEF, 0xFFFFFFFF):
        for iters in (1, 4, 64):
            r, t = ref.healthy_sweep(16, nonce, iters, ref.spread_placement(16, 8))
            others = [(f"tiles_of_iters_{it}", [(TILES, e, int(w)) for e, w in enumerate(
                ref.sweep_tiles(nonce, it, 16).reshape(-1).view(np.uint32))], {"ok": False, "records_ok": 0})
                for it in (1, 4, 64) if it != iters]
            cases[f"sweep16_{nonce:08x}_{iters}"] = Case(
                "sweep", (r, t), dict(grid=16, nonce=nonce, iters=iters, num_xcc=8), healthy(16, 8), others)

    # placement and timing, 64 workgroups over 8 XCDs
    g = 64
    place = ref.spread_placement(g, 8)
    r, t = ref.healthy_sweep(g, NONCE, ITERS, place)
    hw = lambda wg: int(r[wg, ref.REC_HWID])  # noqa: E731
    t_lo, t_hi = 0xFFFFFFF0, 0x1_0000_0010
    variants = [
        # workgroups 5 and 13 are both on XCD 5
        ("same_cu_key", [(RECORDS, rec_word(5, ref.REC_HWID), hw(13))], {"ok": True, "cus_covered": g - 1}),
        ("hwid_differs_outside_15_8", [(RECORDS, rec_word(5, ref.REC_HWID), (hw(13) & 0xFF00) | 0xABCD00EF)],
         {"ok": True, "cus_covered": g - 1}),
        ("hwid_noise_outside_15_8", [(RECORDS, rec_word(w, ref.REC_HWID), hw(w) | (0x9E370000 * (w + 1) & 0xFFFF0000)
                                      | (w * 37 & 0xFF)) for w in range(g)], {"ok": True, "cus_covered": g}),
        ("xcc_high_bits", [(RECORDS, rec_word(w, ref.REC_XCC), int(r[w, ref.REC_XCC]) | 0xFFFFFFF0 & ~(w << 4))
                           for w in range(g)],
         {"ok": True, "xccs_covered": 8, "cus_covered": g, "wgs_per_xcc": [8] * 8}),
        ("one_arrived_short", [(RECORDS, rec_word(9, ref.REC_ARRIVED), g - 1)], {"ok": True, "all_resident": False}),
        ("arrivals_either_side_of_2^32",
         [(RECORDS, rec_word(w, ref.REC_T0_LO), (t_hi if w == 40 else t_lo) & M32) for w in range(g)]
         + [(RECORDS, rec_word(w, ref.REC_T0_HI), (t_hi if w == 40 else t_lo) >> 32) for w in range(g)],
         {"ok": True, "arrival_spread_us": 0.32}),
    ]
    cases["sweep64_placement"] = Case("sweep", (r, t), dict(grid=g, nonce=NONCE, iters=ITERS, num_xcc=8),
                                      dict(healthy(g, 8), arrival_spread_us=0.63), variants)
    seven = [(x if x < 7 else 6, cu if x < 7 else cu + 8) for x, cu in place]      # XCD 7's share runs on XCD 6
    r7, t7 = ref.healthy_sweep(g, NONCE, ITERS, seven)
    cases["sweep64_seven_xcds_of_8"] = Case("sweep", (r7, t7), dict(grid=g, nonce=NONCE, iters=ITERS, num_xcc=8),
                                            {"ok": False, "records_ok": g, "xccs_covered": 7, "cus_covered": g,
                                             "wgs_per_xcc": [8] * 6 + [16, 0]})
    cases["sweep64_seven_xcds_unknown"] = Case("sweep", (r7.copy(), t7.copy()),
                                               dict(grid=g, nonce=NONCE, iters=ITERS, num_xcc=0),
                                               {"ok": True, "records_ok": g, "xccs_covered": 7})
    return cases


ONE = 0x3F800000            # 1.0f
TIMES = dict(fill_us=812.3, check_us=701.7, check2_us=655.0, mfma_us=20011.3)


def _burn_placement(wgs, xcds, cus):
    return [(wg % xcds, (wg // xcds) % cus) for wg in range(wgs)]


def _perf_cases():
    cases = {}
    g = 512
    params = dict(burn_wgs=g, nonce=NONCE, num_xcc=8, bytes=4 * GIB, mfma_iters=1 << 16, **TIMES)
    checksum = 0x42F6E979
    recs = ref.healthy_burn(g, NONCE, _burn_placement(g, 8, 32), 2_400_123, 100_000, checksum)
    healthy = {"ok": True, "hbm_bad_words": 0, "hbm_bad_words_pass2": 0, "hbm_first_bad": -1, "mfma_records_ok": g,
               "mfma_checksum_mismatch": 0, "mfma_xccs": 8, "xcd_clock_mhz": [2400] * 8}
    gone = {"ok": False, "mfma_records_ok": g - 1, "mfma_checksum_mismatch": 0, "mfma_xccs": 8, "hbm_bad_words": 0}
    n16 = 4 * GIB // 16
    variants = [
        ("last_wave_one_bit", [(RECORDS, rec_word(g - 1, ref.PREC_SUM + 3), checksum ^ 1)],
         {"ok": False, "mfma_checksum_mismatch": 1, "mfma_records_ok": g}),
        ("wg0_wave0_differs", [(RECORDS, rec_word(0, ref.PREC_SUM), checksum ^ 0x00400000)],
         {"ok": False, "mfma_checksum_mismatch": 4 * g - 1, "mfma_records_ok": g}),
        ("wg0_absent_reference_is_wg1", [(RECORDS, rec_word(0, ref.PREC_MAGIC), 0),
                                         (RECORDS, rec_word(0, ref.PREC_SUM), checksum ^ 2)], gone),
        ("all_nan", [(RECORDS, rec_word(w, ref.PREC_SUM + v), 0x7FC00000) for w in range(g) for v in range(4)],
         {"ok": False, "mfma_checksum_mismatch": 4 * g, "mfma_records_ok": g}),
        ("all_inf", [(RECORDS, rec_word(w, ref.PREC_SUM + v), 0x7F800000) for w in range(g) for v in range(4)],
         {"ok": False, "mfma_checksum_mismatch": 4 * g, "mfma_records_ok": g}),
        ("all_minus_inf", [(RECORDS, rec_word(w, ref.PREC_SUM + v), 0xFF800000) for w in range(g) for v in range(4)],
         {"ok": False, "mfma_checksum_mismatch": 4 * g}),
        ("all_largest_finite", [(RECORDS, rec_word(w, ref.PREC_SUM + v), 0x7F7FFFFF) for w in range(g)
                                for v in range(4)], {"ok": True, "mfma_checksum_mismatch": 0}),
    ]
    for w in (0, 37, g - 1):
        variants += [
            (f"zero_record@{w}", [(RECORDS, rec_word(w, k), 0) for k in range(16)], gone),
            (f"magic@{w}", [(RECORDS, rec_word(w, ref.PREC_MAGIC), ref.PERF_MAGIC ^ 0x100)], gone),
            (f"wrong_wg@{w}", [(RECORDS, rec_word(w, ref.PREC_WG), w ^ 1)], gone),
            (f"wrong_nonce@{w}", [(RECORDS, rec_word(w, ref.PREC_NONCE), (NONCE ^ w) + 1 & M32)], gone),
            (f"no_interval@{w}", [(RECORDS, rec_word(w, ref.PREC_RT1_LO), int(recs[w, ref.PREC_RT0_LO])),
                                  (RECORDS, rec_word(w, ref.PREC_RT1_HI), int(recs[w, ref.PREC_RT0_HI]))],
             {"ok": True, "mfma_records_ok": g, "mfma_xccs": 8}),
        ]
    counters = lambda *c: [(COUNTERS, i, v) for i, v in enumerate(c)]  # noqa: E731
    variants += [
        ("one_bad_word_pass1", counters(1, 0, 700, 0),
         {"ok": False, "hbm_bad_words": 1, "hbm_bad_words_pass2": 0, "hbm_first_bad": 700}),
        ("three_bad_words_pass2", counters(0, 3, 700, 0),
         {"ok": False, "hbm_bad_words": 3, "hbm_bad_words_pass2": 3, "hbm_first_bad": 700}),
        ("pass1_found_more", counters(5, 3, 0, 0),
         {"ok": False, "hbm_bad_words": 5, "hbm_bad_words_pass2": 3, "hbm_first_bad": 0}),
        ("last_unit", counters(1, 1, n16 - 1, 0), {"ok": False, "hbm_first_bad": n16 - 1}),
        ("first_bad_past_the_buffer", counters(1, 1, n16, 0), {"ok": False, "hbm_first_bad": -1}),
        ("counters_at_the_fill", counters(*[ref.COUNTER_FILL_WORD] * 4),
         {"ok": False, "hbm_first_bad": -1, "hbm_bad_words": ref.COUNTER_FILL_WORD,
          "hbm_bad_words_pass2": ref.COUNTER_FILL_WORD}),
    ]
    cases["burn512"] = Case("perf", (recs, np.array(CLEAN, dtype=np.uint32)), params, healthy, variants)

    # 128 GiB: a first bad unit whose high word counts
    big = dict(params, burn_wgs=2, num_xcc=0, bytes=128 * GIB)
    r2 = ref.healthy_burn(2, NONCE, [(3, 0), (3, 1)], 2_400_000, 100_000, checksum)
    cases["burn2_first_bad_high_word"] = Case(
        "perf", (r2, np.array([1, 0, 2, 1], dtype=np.uint32)), big,
        {"ok": False, "hbm_bad_words": 1, "hbm_first_bad": 0x1_0000_0002, "mfma_xccs": 1},
        [("low_word_only_would_be_2", [(COUNTERS, 3, 0)], {"hbm_first_bad": 2})])

    # 2 workgroups, no XCD count; +0.0 checksums
    small = dict(burn_wgs=2, nonce=1, num_xcc=0, bytes=GIB, mfma_iters=3, **TIMES)
    rz = ref.healthy_burn(2, 1, [(0, 0), (0, 0)], 240_000, 10_000, 0)
    cases["burn2_zero_checksum"] = Case(
        "perf", (rz, np.array(CLEAN, dtype=np.uint32)), small,
        {"ok": True, "mfma_records_ok": 2, "mfma_xccs": 1, "mfma_checksum_mismatch": 0, "clock_mhz_median": 2400},
        [("negative_zero_wave", [(RECORDS, rec_word(1, ref.PREC_SUM + 2), 0x80000000)],
          {"ok": False, "mfma_checksum_mismatch": 1}),
         ("negative_zero_reference", [(RECORDS, rec_word(0, ref.PREC_SUM), 0x80000000)],
          {"ok": False, "mfma_checksum_mismatch": 7})])

    # one XCD absent, 64 workgroups
    seven = [(x if x < 7 else 6, cu) for x, cu in _burn_placement(64, 8, 4)]
    r7 = ref.healthy_burn(64, NONCE, seven, 2_400_000, 100_000, checksum)
    p7 = dict(params, burn_wgs=64)
    cases["burn64_seven_xcds_of_8"] = Case("perf", (r7, np.array(CLEAN, dtype=np.uint32)), p7,
                                           {"ok": False, "mfma_xccs": 7, "mfma_records_ok": 64,
                                            "mfma_checksum_mismatch": 0, "xcd_clock_mhz": [2400] * 7 + [0]})
    cases["burn64_seven_xcds_unknown"] = Case("perf", (r7.copy(), np.array(CLEAN, dtype=np.uint32)),
                                              dict(p7, num_xcc=0), {"ok": True, "mfma_xccs": 7})

    # clocks: XCD x runs 2 + x % 3 workgroups (even and odd counts), each at its own clock, listed
    # out of order, XCC ids up to 15
    place, mhz = [], []
    for x in range(16):
        n = 2 + x % 3
        place += [(x, k) for k in range(n)]
        mhz += [1000 + 60 * x + 7 * ((k * 3 + 1) % n) for k in range(n)]
    gc = len(place)
    rc = ref.healthy_burn(gc, 5, place, [m * 1000 + 300 for m in mhz], 100_000, checksum)
    by_xcd = [sorted(m for (x, _), m in zip(place, mhz) if x == xcd) for xcd in range(16)]
    assert all(c[len(c) // 2] != c[(len(c) - 1) // 2] for c in by_xcd if len(c) % 2 == 0)
    first_of_15 = place.index((15, 0))
    cases["burn_clocks_16_xcds"] = Case(
        "perf", (rc, np.array(CLEAN, dtype=np.uint32)), dict(params, burn_wgs=gc, nonce=5, num_xcc=16),
        {"ok": True, "mfma_xccs": 16, "xcd_clock_mhz": [c[len(c) // 2] for c in by_xcd], "clock_mhz_min": 1000,
         "clock_mhz_max": max(mhz), "clock_mhz_median": sorted(mhz)[gc // 2]},
        [("xcd15_one_record_without_interval",
          [(RECORDS, rec_word(first_of_15, ref.PREC_RT1_LO), int(rc[first_of_15, ref.PREC_RT0_LO])),
           (RECORDS, rec_word(first_of_15, ref.PREC_RT1_HI), int(rc[first_of_15, ref.PREC_RT0_HI]))],
          {"ok": True, "mfma_records_ok": gc, "mfma_xccs": 16}),
         ("xcd15_interval_backwards", [(RECORDS, rec_word(first_of_15, ref.PREC_RT1_HI), 0)],
          {"ok": True, "mfma_records_ok": gc}),
         ("cycles_use_their_high_word", [(RECORDS, rec_word(0, ref.PREC_CYC_HI), 1)],
          {"ok": True, "clock_mhz_max": 4295975})])

    # rates
    rr = ref.healthy_burn(2, 1, [(0, 0), (1, 0)], 240_000, 10_000, ONE)
    for name, times, expect in (
            ("second_pass_untimed", dict(TIMES, check2_us=0.0), {"hbm_read_gbps": 1530.2}),
            ("second_pass_slower", dict(TIMES, check2_us=913.3), {"hbm_read_gbps": 1530.2}),
            ("second_pass_faster", TIMES, {"hbm_read_gbps": 1639.3}),
            ("first_pass_untimed", dict(TIMES, check_us=0.0), {"hbm_read_gbps": 1639.3}),
            ("no_times", dict(fill_us=0.0, check_us=0.0, check2_us=0.0, mfma_us=0.0),
             {"hbm_read_gbps": 0, "hbm_write_gbps": 0, "mfma_tflops": 0})):
        cases[f"burn2_rates_{name}"] = Case("perf", (rr.copy(), np.array(CLEAN, dtype=np.uint32)),
                                            dict(small, num_xcc=2, **times), dict(expect, ok=True))
    return cases


SWEEP_NAMES = (["sweep256"] + [f"sweep256_tile{w}_bits" for w in WGS] + ["sweep32_one_xcd", "sweep4_no_xcd_count"]
               + [f"sweep16_{n:08x}_{it}" for n in (0, 0xDEADBEEF, 0xFFFFFFFF) for it in (1, 4, 64)]
               + ["sweep64_placement", "sweep64_seven_xcds_of_8", "sweep64_seven_xcds_unknown"])
PERF_NAMES = (["burn512", "burn2_first_bad_high_word", "burn2_zero_checksum", "burn64_seven_xcds_of_8",
               "burn64_seven_xcds_unknown", "burn_clocks_16_xcds"]
              + [f"burn2_rates_{n}" for n in ("second_pass_untimed", "second_pass_slower", "second_pass_faster",
                                              "first_pass_untimed", "no_times")])


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.contract_cli(tmp_path_factory.mktemp("kernel_contract"))


@pytest.fixture(scope="module")
def corpus():
    cases = {**_sweep_cases(), **_perf_cases()}
    assert list(cases) == SWEEP_NAMES + PERF_NAMES
    return cases


class Lines:
    """The raw output lines of one program over the whole corpus, per case: one
    process per case, a few at a time."""

    def __init__(self, cli, corpus):
        def one(name):
            case = corpus[name]
            return contract_cli.run_lines(cli, f"{case.kind}-verdict", case.blob(), len(case.variants))
        names = SWEEP_NAMES + PERF_NAMES
        with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
            self.by_case = dict(zip(names, pool.map(one, names)))


@pytest.fixture(scope="module")
def lines(cli, corpus):
    return Lines(cli, corpus)


# ---- every line against the reference ------------------------------------------------------------
def _sweep_error(d):
    return (f"{d['records_ok']}/{d['grid']} workgroups correct (mfma_bad={d['mfma_bad']} lds_bad={d['lds_bad']} "
            f"tile_bad={d['tile_bad']}), {d['xccs_covered']}/{d['num_xcc']} XCDs ran")


def _perf_error(d):
    return (f"hbm_bad_words={d['hbm_bad_words']} first_bad_unit={d['hbm_first_bad']} mfma records "
            f"{d['mfma_records_ok']}/{d['mfma_grid']} checksum mismatches {d['mfma_checksum_mismatch']}, "
            f"{d['mfma_xccs']}/{d['num_xcc']} XCDs ran")


def _check_case(case, raw_lines):
    sweep = case.kind == "sweep"
    digits = ref.SWEEP_FLOAT_DIGITS if sweep else ref.PERF_FLOAT_DIGITS
    zero_keys = SWEEP_ZERO_KEYS if sweep else PERF_ZERO_KEYS
    arrays = case.words()
    assert len(raw_lines) == len(case.variants)
    for (label, patches, expect), line in zip(case.variants, raw_lines):
        got = json.loads(line)
        saved = [(a, i, int(arrays[a][i])) for a, i, _ in patches]
        for a, i, v in patches:
            arrays[a][i] = v & M32
        want = case.reference()
        for a, i, v in reversed(saved):
            arrays[a][i] = v
        ref.assert_verdict(got, want, digits, label)
        assert set(got) == set(want) | set(zero_keys) | {"error"}, label
        for key, value in zero_keys.items():
            assert got[key] == value, (label, key, got[key])
        for key, value in expect.items():           # what this variant is there to show
            if key in digits:
                ref.assert_verdict(got, {key: value}, digits, label)
            else:
                assert got[key] == value and type(got[key]) is type(value), (label, key, got[key], value)
        if got["ok"]:
            assert got["error"] == "", (label, got["error"])
        elif sweep:
            assert got["error"] == _sweep_error(want), (label, got["error"])
        else:
            assert got["error"].startswith(_perf_error(want)), (label, got["error"])
            tail = got["error"][len(_perf_error(want)):]
            assert tail in ("", "; HBM counters were not copied"), (label, got["error"])


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_sweep_verdict_equals_the_reference(corpus, lines, name):
    _check_case(corpus[name], lines.by_case[name])


@pytest.mark.parametrize("name", PERF_NAMES)
def test_perf_verdict_equals_the_reference(corpus, lines, name):
    _check_case(corpus[name], lines.by_case[name])


def test_corpus_holds_the_cases_it_should(corpus):
    labels = [lb for lb, _, _ in corpus["sweep256"].variants]
    for w in WGS:
        for kind in ("magic", "wg_off_by_one", "zero_record", "mfma_bad", "lds_bad", "absent_with_mfma_bad",
                     "negative_zero", "tiles_exchanged", "tile_at_prefill"):
            assert f"{kind}@{w}" in labels
        assert (f"nonce_sum@{w}" in labels) == (w != 0)          # nonce + 0 is nonce ^ 0
        assert sum(lb.startswith(f"tile{w}[0]^bit") for lb in labels) == 32
        assert len(corpus[f"sweep256_tile{w}_bits"].variants) == 1 + 1024 * 2


def test_unwritten_counters_are_named_in_the_error(corpus, lines):
    case = corpus["burn512"]
    by_label = {lb: json.loads(ln) for (lb, _, _), ln in zip(case.variants, lines.by_case["burn512"])}
    assert by_label["counters_at_the_fill"]["error"].endswith("; HBM counters were not copied")
    assert by_label["first_bad_past_the_buffer"]["error"].endswith("; HBM counters were not copied")
    for label in ("one_bad_word_pass1", "three_bad_words_pass2", "last_unit", "zero_record@0", "all_nan"):
        assert by_label[label]["error"].endswith("XCDs ran"), by_label[label]["error"]


# ---- the JSON line itself ----------------------------------------------------------------------
def _c_format(fmt, values):
    """A printf format of ints, doubles and strings through Python's % operator."""
    return fmt.replace("%llu", "%d").replace("%lld", "%d").replace("%u", "%d") % tuple(values)


def _json_bool(b):
    return "true" if b else "false"


def _without_identity(line):
    """The line as it was before a check's reply named its agent: the two keys
    in front of "error", which a verdict on records alone leaves at -1 and ""."""
    key = ",\"kfd_node_id\":-1,\"pci_bus_id\":\"\",\"error\":"
    assert line.count(key) == 1, line[-200:]
    return line.replace(key, ",\"error\":")


def test_json_line_is_byte_identical_to_the_fixed_buffer_format(corpus, lines):
    w = corpus["sweep256"].reference()
    per = "[" + ",".join(str(x) for x in w["wgs_per_xcc"]) + "]"
    assert _without_identity(lines.by_case["sweep256"][0]) == _c_format(OLD_SWEEP_FORMAT, [
        0, _json_bool(w["ok"]), 0, w["nonce"], w["iters"], w["grid"], 0, w["num_xcc"], w["records_ok"], w["mfma_bad"],
        w["lds_bad"], w["tile_bad"], w["cus_covered"], w["xccs_covered"], _json_bool(w["all_resident"]), per, 0.0,
        w["arrival_spread_us"], 0.0, 0.0, "false", ""])
    for name in ("burn512", "burn_clocks_16_xcds"):
        w = corpus[name].reference()
        per = "[" + ",".join("%.0f" % x for x in w["xcd_clock_mhz"]) + "]"
        assert _without_identity(lines.by_case[name][0]) == _c_format(OLD_PERF_FORMAT, [
            0, _json_bool(w["ok"]), 0, w["nonce"], w["bytes"], 0, w["num_xcc"], w["fill_us"], w["check_us"],
            w["check2_us"], w["hbm_write_gbps"], w["hbm_read_gbps"], w["hbm_bad_words"], w["hbm_bad_words_pass2"],
            w["hbm_first_bad"], w["mfma_iters"], w["mfma_grid"], w["mfma_records_ok"], w["mfma_checksum_mismatch"],
            w["mfma_xccs"], w["mfma_us"], w["mfma_tflops"], w["clock_mhz_min"], w["clock_mhz_median"],
            w["clock_mhz_max"], per, 0.0, 0.0, "false", ""])


WIDE_ERROR = (b"\"\\\x01\x1f\n\t\r\x08\x0c" * 18)[:159]
WIDE = dict(i=-2 ** 31, u32=2 ** 32 - 1, u64=2 ** 64 - 1, i64=-2 ** 63, d=1e15)


def _wide_line(cli, kind, i=None):
    args = [str(WIDE["i"] if i is None else i), str(WIDE["u32"]), str(WIDE["u64"]), str(WIDE["i64"]), "1e15",
            WIDE_ERROR.hex()]
    r = subprocess.run([str(cli), "json", kind] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.endswith("}\n") and r.stdout.count("\n") == 1
    return r.stdout[:-1]


@pytest.mark.parametrize("kind", ["sweep", "perf"])
def test_json_line_with_every_field_at_its_widest_is_whole(cli, kind):
    assert len(WIDE_ERROR) == 159 and all(b in b"\"\\" or b < 0x20 for b in WIDE_ERROR)
    line = _wide_line(cli, kind)
    assert len(line) > (1024 if kind == "sweep" else 1536)          # the buffers it once had to fit
    d = json.loads(line)
    assert d["error"] == WIDE_ERROR.decode()
    ints = {"sweep": ("ordinal", "hsa_error", "iters", "grid", "cu_count", "num_xcc", "records_ok", "cus_covered",
                      "xccs_covered"),
            "perf": ("ordinal", "hsa_error", "cu_count", "num_xcc", "mfma_iters", "mfma_grid", "mfma_records_ok",
                     "mfma_checksum_mismatch", "mfma_xccs")}[kind]
    floats = {"sweep": ("kernel_us", "arrival_spread_us", "total_us", "in_flight_s"),
              "perf": ("fill_us", "check_us", "check2_us", "hbm_write_gbps", "hbm_read_gbps", "mfma_us", "mfma_tflops",
                       "total_us", "in_flight_s")}[kind]
    assert all(d[k] == WIDE["i"] for k in ints) and all(d[k] == 1e15 for k in floats)
    assert d["nonce"] == WIDE["u32"] and d["ok"] is True and d["kept_queue"] is True
    assert d["kfd_node_id"] == WIDE["i"] and d["pci_bus_id"] == WIDE_ERROR[:31].decode()
    if kind == "sweep":
        assert d["mfma_bad"] == d["lds_bad"] == d["tile_bad"] == WIDE["u32"] and d["all_resident"] is True
        assert d["wgs_per_xcc"] == [WIDE["i"]] * 8
    else:
        assert d["bytes"] == d["hbm_bad_words"] == d["hbm_bad_words_pass2"] == WIDE["u64"]
        assert d["hbm_first_bad"] == WIDE["i64"]
        assert d["xcd_clock_mhz"] == [1e15] * 8
        assert all(d[k] == 1e15 for k in ("clock_mhz_min", "clock_mhz_median", "clock_mhz_max"))
    # sixteen per-XCD entries at the largest positive int
    d16 = json.loads(_wide_line(cli, kind, i=2 ** 31 - 1))
    assert len(d16["wgs_per_xcc" if kind == "sweep" else "xcd_clock_mhz"]) == 16 and d16["error"] == d["error"]


# ---- the same corpus through an instrumented build ---------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _sanitizers_link(tmp):
    cxx = contract_cli.host_compiler()
    if not cxx:
        return "no host C++ compiler"
    src = tmp / "one.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SANITIZE, str(src), "-o", str(tmp / "one")], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        return f"a one-line program does not link with {SANITIZE[0]}: {r.stderr[-300:]}"
    r = subprocess.run([str(tmp / "one")], capture_output=True, text=True, timeout=60)
    return None if r.returncode == 0 else f"a one-line program built with {SANITIZE[0]} does not run: {r.stderr[-300:]}"


def test_corpus_through_the_address_and_undefined_sanitizers(corpus, lines, cli, tmp_path):
    """wgs_per_xcc[x], per_xcd[x] and 1u << x are indexed by a record word; the
    corpus holds XCC words with every high bit set and ids up to 15."""
    reason = _sanitizers_link(tmp_path)
    if reason:
        pytest.skip(reason)
    exe = contract_cli.compile_cli(tmp_path / "kernel_contract_cli_san", SANITIZE)
    checked = Lines(exe, corpus)
    for name in SWEEP_NAMES + PERF_NAMES:
        assert checked.by_case[name] == lines.by_case[name], name
    for kind in ("sweep", "perf"):
        assert _wide_line(exe, kind) == _wide_line(cli, kind)
