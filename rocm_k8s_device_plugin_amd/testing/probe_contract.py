"""What each fault mode of testing/stub_probe.py stands for, as the records a
GPU would have left behind, and the shipped host verdict on them.

The stub answers a sweep, a throughput check or a datapath check with figures
written into its source. They are true figures only if the real verdict
(chip_verify.h, datapath_verify.h, datapath_i8_verify.h, datapath_bf16_verify.h,
datapath_fp8_verify.h, datapath_f16_verify.h, datapath_f64_verify.h, datapath_f6f4_verify.h,
datapath_sparse_verify.h, datapath_gemm_verify.h, datapath_splitk_verify.h,
datapath_attn_verify.h) says the same of the
fault the mode names, so every mode is defined here as a change to healthy
records (testing/kernel_reference.py, datapath_reference.py and
datapath_i8_reference.py build those), and `real_replies` runs the contract
programs on them. tests/test_probe_contract.py compares the two.

The stub does not compute: its figures are those of NONCE, ITERS and GRID
below, whatever nonce it is asked with (it echoes the request's).
"""
from __future__ import annotations

import json

import numpy as np

from . import contract_cli
from . import datapath_bf16_reference as dpbf
from . import datapath_fp8_reference as dpf8
from . import datapath_f16_reference as dphf
from . import datapath_f64_reference as dpd
from . import datapath_f6f4_reference as dpf6
from . import datapath_i8_reference as dpi8
from . import datapath_sparse_reference as dpsp
from . import datapath_gemm_reference as dpgm
from . import datapath_splitk_reference as dpsk
from . import datapath_attn_reference as dpat
from . import datapath_mxgemm_reference as dpmx
from . import datapath_mxquant_reference as dpmq
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
        "datapath_bf16": DATAPATH_KEYS, "datapath_fp8": DATAPATH_KEYS, "datapath_f16": DATAPATH_KEYS,
        "datapath_f64": DATAPATH_KEYS, "datapath_f6f4": DATAPATH_KEYS, "datapath_sparse": DATAPATH_KEYS,
        "datapath_gemm": DATAPATH_KEYS, "datapath_splitk": DATAPATH_KEYS + ("tiles", "splits", "ledger_bad"),
        "datapath_attn": DATAPATH_KEYS + ("heads", "qblocks", "kblocks", "exp_inexact"),
        "datapath_mxgemm": DATAPATH_KEYS + ("ksteps",), "datapath_mxquant": DATAPATH_KEYS + ("hsteps",)}
MODES = {"sweep": SWEEP_MODES, "perf": PERF_MODES, "datapath": DATAPATH_MODES, "datapath_i8": DATAPATH_MODES,
         "datapath_bf16": DATAPATH_MODES, "datapath_fp8": DATAPATH_MODES, "datapath_f16": DATAPATH_MODES,
         "datapath_f64": DATAPATH_MODES, "datapath_f6f4": DATAPATH_MODES, "datapath_sparse": DATAPATH_MODES,
         "datapath_gemm": DATAPATH_MODES, "datapath_splitk": DATAPATH_MODES, "datapath_attn": DATAPATH_MODES,
         "datapath_mxgemm": DATAPATH_MODES, "datapath_mxquant": DATAPATH_MODES}

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


def datapath_f64_replies(build_dir) -> list:
    """As _datapath_case, on stage 3 (the sum stage, 512 words): the shipped verdict's device objects for the
    modes, on the header's own image (datapath_f64_contract_cli image)."""
    cli = contract_cli.datapath_f64_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_f64_image(cli, GRID, NONCE), dtype="<u4")
    out = []
    for mode in MODES["datapath_f64"]:
        recs = healthy[:GRID * dpd.REC_WORDS].reshape(GRID, dpd.REC_WORDS).copy()
        tiles = healthy[GRID * dpd.REC_WORDS:].reshape(GRID, dpd.WG_WORDS).copy()
        lo = dpd.TILE_OFFSET[3]
        if mode == "stuck_bit":
            tiles[WG, lo:lo + dpd.STAGE_WORDS[3]] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpd.REC_BAD + 3] = 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_f64_verdict(cli, dpd.image_bytes(recs, tiles), GRID, NONCE, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_f6f4_replies(build_dir) -> list:
    """As _datapath_case, on stage 4 (the first product stage, 1024 words): the shipped verdict's device objects for the
    modes, on the header's own image (datapath_f6f4_contract_cli image)."""
    cli = contract_cli.datapath_f6f4_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_f6f4_image(cli, GRID, NONCE), dtype="<u4")
    out = []
    for mode in MODES["datapath_f6f4"]:
        recs = healthy[:GRID * dpf6.REC_WORDS].reshape(GRID, dpf6.REC_WORDS).copy()
        tiles = healthy[GRID * dpf6.REC_WORDS:].reshape(GRID, dpf6.WG_WORDS).copy()
        lo = dpf6.TILE_OFFSET[4]
        if mode == "stuck_bit":
            tiles[WG, lo:lo + dpf6.STAGE_WORDS[4]] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpf6.REC_BAD + 4] = 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_f6f4_verdict(cli, dpf6.image_bytes(recs, tiles), GRID, NONCE, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_sparse_replies(build_dir) -> list:
    """As _datapath_case, on stage 3 (the first sum stage, 1024 words): the shipped verdict's device objects for the
    modes, on the header's own image (datapath_sparse_contract_cli image)."""
    cli = contract_cli.datapath_sparse_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_sparse_image(cli, GRID, NONCE), dtype="<u4")
    out = []
    for mode in MODES["datapath_sparse"]:
        recs = healthy[:GRID * dpsp.REC_WORDS].reshape(GRID, dpsp.REC_WORDS).copy()
        tiles = healthy[GRID * dpsp.REC_WORDS:].reshape(GRID, dpsp.WG_WORDS).copy()
        lo = dpsp.TILE_OFFSET[3]
        if mode == "stuck_bit":
            tiles[WG, lo:lo + dpsp.STAGE_WORDS[3]] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpsp.REC_BAD + 3] = 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_sparse_verdict(cli, dpsp.image_bytes(recs, tiles), GRID, NONCE, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_gemm_replies(build_dir) -> list:
    """As _datapath_case for the GEMM pipeline check at the production K: the shipped verdict's device objects for the
    modes, on the header's own image. stuck_bit: bit 30 of every D word of row 0 of one workgroup; device_bad: that
    workgroup's first A fold word is off by 12."""
    cli = contract_cli.datapath_gemm_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_gemm_image(cli, GRID, NONCE, dpgm.KSTEPS), dtype="<u4")
    out = []
    for mode in MODES["datapath_gemm"]:
        recs = healthy[:GRID * dpgm.REC_WORDS].reshape(GRID, dpgm.REC_WORDS).copy()
        tiles = healthy[GRID * dpgm.REC_WORDS:].reshape(GRID, dpgm.WG_WORDS).copy()
        if mode == "stuck_bit":
            tiles[WG, :dpgm.TILE] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpgm.fold_slot(0, 1)] += 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_gemm_verdict(cli, dpgm.image_bytes(recs, tiles), GRID, NONCE, dpgm.KSTEPS, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_mxgemm_replies(build_dir) -> list:
    """As datapath_gemm_replies for the MXFP4 GEMM pipeline check at the production K: stuck_bit is bit 30 of every D
    word of row 0 of one workgroup; device_bad: that workgroup's first A fold sum is off by 12."""
    cli = contract_cli.datapath_mxgemm_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_mxgemm_image(cli, GRID, NONCE, dpmx.KSTEPS), dtype="<u4")
    out = []
    for mode in MODES["datapath_mxgemm"]:
        recs = healthy[:GRID * dpmx.REC_WORDS].reshape(GRID, dpmx.REC_WORDS).copy()
        tiles = healthy[GRID * dpmx.REC_WORDS:].reshape(GRID, dpmx.WG_WORDS).copy()
        if mode == "stuck_bit":
            tiles[WG, :dpmx.TILE] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpmx.fold_slot(0, 1)] += 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_mxgemm_verdict(cli, dpmx.image_bytes(recs, tiles), GRID, NONCE, dpmx.KSTEPS, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_mxquant_replies(build_dir) -> list:
    """As datapath_mxgemm_replies for the MX quantise check at the production shape: stuck_bit is bit 30 of every Y word
    of row 0 of one workgroup; device_bad: that workgroup's first W1 fold sum is off by 12."""
    cli = contract_cli.datapath_mxquant_cli(build_dir)
    healthy = np.frombuffer(contract_cli.datapath_mxquant_image(cli, GRID, NONCE, dpmq.HSTEPS), dtype="<u4")
    cut = np.cumsum([GRID * dpmq.REC_WORDS, GRID * dpmq.img_words(dpmq.HSTEPS)])
    out = []
    for mode in MODES["datapath_mxquant"]:
        recs, images, tiles = (part.reshape(GRID, -1).copy() for part in np.split(healthy, cut))
        if mode == "stuck_bit":
            tiles[WG, :dpmq.TILE] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs[WG, dpmq.fold_slot(0, 1)] += 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_mxquant_verdict(cli, dpmq.image_bytes(recs, images, tiles), GRID, NONCE, dpmq.HSTEPS,
                                                  build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_splitk_replies(build_dir) -> list:
    """As datapath_gemm_replies for the split-K check at the production sizes (GRID / 8 tiles, 8 splits of 4 k-steps).
    stuck_bit: bit 30 of every D word of row 0 of tile WG; missing: workgroups WG and WG + 1 (both of tile WG // 8)
    wrote no record; device_bad: workgroup WG's first A fold sum is off by 12."""
    cli = contract_cli.datapath_splitk_cli(build_dir)
    tiles, sizes = GRID // dpsk.CUS_PER_TILE, (GRID // dpsk.CUS_PER_TILE, dpsk.SPLITS, dpsk.KSTEPS, NONCE)
    healthy = np.frombuffer(contract_cli.datapath_splitk_image(cli, *sizes), dtype="<u4")
    out = []
    for mode in MODES["datapath_splitk"]:
        recs, d, led = (x.copy() for x in np.split(healthy, [GRID * dpsk.REC_WORDS, GRID * dpsk.REC_WORDS + tiles * dpsk.TILE_WORDS]))
        if mode == "stuck_bit":
            d.reshape(tiles, dpsk.TILE_WORDS)[WG, :dpsk.TILE] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs.reshape(GRID, dpsk.REC_WORDS)[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs.reshape(GRID, dpsk.REC_WORDS)[WG, dpsk.fold_slot(0, 1)] += 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_splitk_verdict(cli, dpsk.image_bytes(recs, d, led), *sizes, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


def datapath_attn_replies(build_dir) -> list:
    """As datapath_gemm_replies for the attention check at the production sizes (GRID / 4 heads, 4 query blocks, 4 key
    blocks). stuck_bit: bit 30 of the 64 O words of query 0 of workgroup WG; missing: workgroups WG and WG + 1 wrote no
    record; device_bad: the first K fold sum of workgroup WG is off by 12."""
    cli = contract_cli.datapath_attn_cli(build_dir)
    sizes = (GRID // dpat.CUS_PER_HEAD, dpat.QBLOCKS, dpat.KBLOCKS, NONCE)
    healthy = np.frombuffer(contract_cli.datapath_attn_image(cli, *sizes), dtype="<u4")
    out = []
    for mode in MODES["datapath_attn"]:
        recs, ml, o = (x.copy() for x in np.split(healthy, [GRID * dpat.REC_WORDS, GRID * (dpat.REC_WORDS + dpat.ML_WORDS)]))
        if mode == "stuck_bit":
            o.reshape(GRID, dpat.O_WORDS)[WG, :dpat.D] &= np.uint32(~(1 << BIT) & 0xFFFFFFFF)
        elif mode == "missing":
            recs.reshape(GRID, dpat.REC_WORDS)[WG:WG + 2, :] = 0
        elif mode == "device_bad":
            recs.reshape(GRID, dpat.REC_WORDS)[WG, dpat.fold_slot(0, 1)] += 12
        else:
            assert mode == "ok", mode
        r = contract_cli.datapath_attn_verdict(cli, dpat.image_bytes(recs, ml, o), *sizes, build_dir)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    return out


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
    elif kind == "datapath_f64":
        out = datapath_f64_replies(build_dir)
    elif kind == "datapath_f6f4":
        out = datapath_f6f4_replies(build_dir)
    elif kind == "datapath_sparse":
        out = datapath_sparse_replies(build_dir)
    elif kind == "datapath_gemm":
        out = datapath_gemm_replies(build_dir)
    elif kind == "datapath_splitk":
        out = datapath_splitk_replies(build_dir)
    elif kind == "datapath_attn":
        out = datapath_attn_replies(build_dir)
    elif kind == "datapath_mxgemm":
        out = datapath_mxgemm_replies(build_dir)
    elif kind == "datapath_mxquant":
        out = datapath_mxquant_replies(build_dir)
    elif kind == "datapath_bf16":
        out = dpbf.verdicts(dpbf.contract_cli(build_dir), [datapath_bf16_case(m) for m in modes], len(modes))
    else:
        out = dpi8.verdicts(dpi8.contract_cli(build_dir), [datapath_i8_case(m) for m in modes], len(modes))
    return dict(zip(modes, out))
