"""What each fault mode of testing/stub_probe.py stands for, as the records a
GPU would have left behind, and the shipped host verdict on them.

The stub answers a sweep, a throughput check or a datapath check with figures
written into its source. They are true figures only if the real verdict
(chip_verify.h, datapath_verify.h, datapath_i8_verify.h, datapath_bf16_verify.h,
datapath_fp8_verify.h, datapath_f16_verify.h) says the same of the
fault the mode names, so every mode is defined here as a change to healthy
records (testing/kernel_reference.py, datapath_reference.py and
datapath_i8_reference.py build those), and `real_replies` runs the contract
programs on them. tests/test_probe_contract.py compares the two.

The stub does not compute: its figures are those of NONCE, ITERS and GRID
below, whatever nonce it is asked with (it echoes the request's).
"""
from __future__ import annotations

import numpy as np

from . import contract_cli
from . import datapath_bf16_reference as dpbf
from . import datapath_fp8_reference as dpf8
from . import datapath_f16_reference as dphf
from . import datapath_i8_reference as dpi8
from . import datapath_reference as dp
from . import kernel_reference as ref

# with this nonce the first word of workgroup WG's tile that has bit BIT set is word 5, in the f32
# check's stage 2 and in the int8 check's stage 4 alike
NONCE, ITERS, GRID, XCDS = 0x5EED142F, 4, 256, 8
BURN_WGS = 2 * GRID                    # MI355X_BURN_WGS_PER_CU workgroups per CU
PERF_BYTES, PERF_ITERS = 4 << 30, 65536
WG = 17                                # the workgroup (one CU) every single-CU fault sits on
BIT = 30                               # the stuck bit (stuck at 0)

SWEEP_MODES = ("ok", "mfma_bad", "lds_bad", "tile_bad", "missing", "missing_xcd")
PERF_MODES = ("ok", "slow_hbm", "slow_mfma", "slow_xcd", "slow_xcd_after_absent", "corrupt")
DATAPATH_MODES = ("ok", "stuck_bit", "missing", "device_bad")

# what the verdict derives from the records (the rest of a reply is the
# device's identity, the request's echo and times)
SWEEP_KEYS = ("ok", "iters", "grid", "num_xcc", "records_ok", "mfma_bad", "lds_bad", "tile_bad", "cus_covered",
              "xccs_covered", "all_resident", "wgs_per_xcc", "error")
PERF_KEYS = ("ok", "bytes", "num_xcc", "hbm_bad_words", "hbm_bad_words_pass2", "hbm_first_bad", "mfma_iters",
             "mfma_grid", "mfma_records_ok", "mfma_checksum_mismatch", "mfma_xccs", "error")
DATAPATH_KEYS = ("ok", "grid", "records_ok", "mfma_bad", "stage_bad", "tile_bad", "first_bad_wg", "first_bad_stage",
                 "first_bad_word", "first_bad_got", "first_bad_want", "first_bad_xor", "cus_covered", "simds_covered",
                 "xccs_covered", "error")
KEYS = {"sweep": SWEEP_KEYS, "perf": PERF_KEYS, "datapath": DATAPATH_KEYS, "datapath_i8": DATAPATH_KEYS,
        "datapath_bf16": DATAPATH_KEYS, "datapath_fp8": DATAPATH_KEYS, "datapath_f16": DATAPATH_KEYS}
MODES = {"sweep": SWEEP_MODES, "perf": PERF_MODES, "datapath": DATAPATH_MODES, "datapath_i8": DATAPATH_MODES,
         "datapath_bf16": DATAPATH_MODES, "datapath_fp8": DATAPATH_MODES, "datapath_f16": DATAPATH_MODES}

# the clocks and times behind the stub's throughput figures (MHz, us)
CLOCK_MHZ, SLOW_XCD, SLOW_XCD_MHZ = 1530, 3, 510
ABSENT_CLOCKS_MHZ = (0, 2400, 2400, 900, 2400)     # slow_xcd_after_absent: XCD 0 reports no clock
RT_TICKS = 100000                                   # 1 ms of the 100 MHz counter


def sweep_case(mode: str) -> bytes:
    xcds = XCDS - 1 if mode == "missing_xcd" else XCDS          # one XCD ran nothing
    recs, tiles = ref.healthy_sweep(GRID, NONCE, ITERS, ref.spread_placement(GRID, xcds))
    if mode == "mfma_bad":
        recs[WG, ref.REC_MFMA_BAD] = 12
    elif mode == "lds_bad":
        recs[WG, ref.REC_LDS_BAD] = 3
    elif mode == "tile_bad":
        tiles.reshape(GRID, -1).view(np.uint32)[WG, 5] ^= np.uint32(1 << BIT)
    elif mode == "missing":
        recs[WG, :] = 0
    else:
        assert mode in ("ok", "missing_xcd"), mode
    return contract_cli.sweep_case(recs, tiles, grid=GRID, nonce=NONCE, iters=ITERS, num_xcc=XCDS)


def perf_case(mode: str) -> bytes:
    """Rates come from the dispatch times, clocks from the records' tick counts."""
    num_xcc = len(ABSENT_CLOCKS_MHZ) if mode == "slow_xcd_after_absent" else XCDS
    placement = ref.spread_placement(BURN_WGS, num_xcc)
    mhz = [CLOCK_MHZ] * num_xcc
    if mode == "slow_xcd":
        mhz[SLOW_XCD] = SLOW_XCD_MHZ
    if mode == "slow_xcd_after_absent":
        mhz = list(ABSENT_CLOCKS_MHZ)
    # an XCD whose workgroups measured no interval reports no clock (0)
    ticks = [RT_TICKS if mhz[x] else 0 for x, _ in placement]
    cyc = [mhz[x] * RT_TICKS // ref.REALTIME_MHZ for x, _ in placement]
    recs = ref.healthy_burn(BURN_WGS, NONCE, placement, cyc, ticks, 0x42C80000)
    counters = [3, 3, 4096, 0] if mode == "corrupt" else [0, 0, ref.M32, ref.M32]
    flops = ref.MFMA_FLOPS * 2 * PERF_ITERS * ref.BURN_WAVES * BURN_WGS
    read_gbps, tflops = (1500.0 if mode == "slow_hbm" else 6000.0), (400.0 if mode == "slow_mfma" else 1550.0)
    return contract_cli.perf_case(recs, counters, burn_wgs=BURN_WGS, nonce=NONCE, num_xcc=num_xcc, bytes=PERF_BYTES,
                                  mfma_iters=PERF_ITERS, fill_us=PERF_BYTES / (4600.0 * 1e3),
                                  check_us=PERF_BYTES / (read_gbps * 1e3), check2_us=PERF_BYTES / (read_gbps * 1e3),
                                  mfma_us=flops / (tflops * 1e6))


def _datapath_case(mod, mode: str, stage: int) -> bytes:
    recs, tiles = mod.healthy(GRID, NONCE)
    if mode == "stuck_bit":            # bit 30 of every word of one CU's stage tile reads 0
        flat = tiles.reshape(GRID, mod.WG_WORDS)
        lo = stage * 1024
        hi = min(lo + 1024, mod.WG_WORDS)
        flat[WG, lo:hi] = mod.stuck_bit(flat[WG, lo:hi], BIT, 0)
    elif mode == "missing":            # two workgroups wrote no record
        recs[WG:WG + 2, :] = 0
    elif mode == "device_bad":         # the device-side compare found mismatches
        recs[WG, mod.REC_BAD + stage] = 12
    else:
        assert mode == "ok", mode
    return mod.case(recs, tiles, GRID, NONCE)


def datapath_case(mode: str) -> bytes:
    return _datapath_case(dp, mode, 1 if mode == "device_bad" else 2)


def datapath_i8_case(mode: str) -> bytes:
    return _datapath_case(dpi8, mode, 4)


def datapath_bf16_case(mode: str) -> bytes:
    return _datapath_case(dpbf, mode, 4)


def datapath_fp8_case(mode: str, image=None) -> bytes:
    """As _datapath_case, on stage 4 (the first scaled stage), whose tile does not start at 4 * 1024.
    `image`: the healthy tiles when the caller has them already (the reference takes half a minute for 256
    workgroups of 64- and 128-term sums in Python integers)."""
    recs, tiles = dpf8.healthy(GRID, NONCE, tiles=image)
    lo = dpf8.TILE_OFFSET[4]
    if mode == "stuck_bit":
        tiles[WG, lo:lo + dpf8.TILE_WORDS[4]] = dpf8.stuck_bit(tiles[WG, lo:lo + dpf8.TILE_WORDS[4]], BIT, 0)
    elif mode == "missing":
        recs[WG:WG + 2, :] = 0
    elif mode == "device_bad":
        recs[WG, dpf8.REC_BAD + 4] = 12
    else:
        assert mode == "ok", mode
    return dpf8.case(recs, tiles, GRID, NONCE)


def datapath_f16_case(mode: str, image=None) -> bytes:
    """As _datapath_case, on stage 4 (the 16x16x32 stage, a tile of 256 words).
    `image`: the healthy tiles when the caller has them already (the reference takes a while for 256
    workgroups in Python integers)."""
    recs, tiles = dphf.healthy(GRID, NONCE, tiles=image)
    lo = dphf.TILE_OFFSET[4]
    if mode == "stuck_bit":
        tiles[WG, lo:lo + dphf.TILE_WORDS[4]] = dphf.stuck_bit(tiles[WG, lo:lo + dphf.TILE_WORDS[4]], BIT, 0)
    elif mode == "missing":
        recs[WG:WG + 2, :] = 0
    elif mode == "device_bad":
        recs[WG, dphf.REC_BAD + 4] = 12
    else:
        assert mode == "ok", mode
    return dphf.case(recs, tiles, GRID, NONCE)


def real_replies(kind: str, build_dir) -> dict:
    """mode -> the device object the shipped verdict and printer give for it."""
    modes = MODES[kind]
    if kind == "sweep":
        out = contract_cli.sweep_verdicts(contract_cli.contract_cli(build_dir), [sweep_case(m) for m in modes], len(modes))
    elif kind == "perf":
        out = contract_cli.perf_verdicts(contract_cli.contract_cli(build_dir), [perf_case(m) for m in modes], len(modes))
    elif kind == "datapath":
        out = dp.verdicts(dp.contract_cli(build_dir), [datapath_case(m) for m in modes], len(modes))
    elif kind == "datapath_fp8":
        cli = dpf8.contract_cli(build_dir)
        # the header's own image for the 255 healthy workgroups; the faulty one's tile is the reference's
        image = dpf8.header_tiles(cli, NONCE, GRID)
        assert (image[WG] == dpf8.tiles_image(NONCE ^ (WG * dpf8.GOLDEN & dpf8.M32), 1)[0]).all()
        out = dpf8.verdicts(cli, [datapath_fp8_case(m, image) for m in modes], len(modes))
    elif kind == "datapath_f16":
        cli = dphf.contract_cli(build_dir)
        # the header's own image for the 255 healthy workgroups; the faulty one's tile is the reference's
        image = dphf.header_tiles(cli, NONCE, GRID)
        assert (image[WG] == dphf.tiles_image(NONCE ^ (WG * dphf.GOLDEN & dphf.M32), 1)[0]).all()
        out = dphf.verdicts(cli, [datapath_f16_case(m, image) for m in modes], len(modes))
    elif kind == "datapath_bf16":
        out = dpbf.verdicts(dpbf.contract_cli(build_dir), [datapath_bf16_case(m) for m in modes], len(modes))
    else:
        out = dpi8.verdicts(dpi8.contract_cli(build_dir), [datapath_i8_case(m) for m in modes], len(modes))
    return dict(zip(modes, out))
