"""Every byte the five kernels of liveness_gfx950.hsaco write, at tiny shapes,
against the independent references of testing/kernel_reference.py.

One child process (testing/raw_kernels.py: ctypes over the ROCm HIP runtime,
no torch) runs one request list; every test asserts on the arrays it saved.
If the child stopped early, the tests whose arrays are missing fail with its
stderr, and nothing else is launched. The comparisons live in
kernel_reference.py; tests/test_kernel_reference.py shows on the CPU that each
of them fails on the output of a wrong kernel.

The same arrays then go through the shipped verdicts (chip_verify.h, by way of
the kernel_contract_cli program the native build produced): what a real kernel
wrote must come out `ok`, equal to the reference verdict field by field, and
stop being `ok` with one bit flipped on the host."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent

LIVE_CASES = [(n, it) for n in ref.NONCES for it in ref.ITERS]
SWEEP_GRID, SWEEP_WAIT_TICKS = 4, 100000
SWEEP_CASES = [(n, it) for n in (0, 0xFFFFFFFF) for it in (1, 4)]

# hbm: 3 workgroups; two passes of the 4x-unrolled loop, one full remainder pass, 5 units more
HBM_GRID, HBM_THREADS = 3, 768
HBM_N16 = 4 * 768 * 2 + 768 + 5
HBM_LAST_UNROLLED = 4 * 768 * 2 - 1
HBM_FIRST_REMAINDER = 4 * 768 * 2
HBM_SEEDS = (0, 0xFFFFFFFF)
FILL_POISONS = {"off": None, "first": 0, "last": HBM_N16 - 1, "remainder": HBM_FIRST_REMAINDER}
FILL_CASES = [(s, p) for s in HBM_SEEDS for p in FILL_POISONS]
# name -> (n16, seed, [(unit, word)] corrupted by the host)
CHECK_CASES = {
    "clean_seed0": (HBM_N16, 0, []),
    "clean": (HBM_N16, 0xFFFFFFFF, []),
    "unit0_word0": (HBM_N16, 0xFFFFFFFF, [(0, 0)]),
    "last_unit_word3": (HBM_N16, 0xFFFFFFFF, [(HBM_N16 - 1, 3)]),
    "last_unrolled": (HBM_N16, 0xFFFFFFFF, [(HBM_LAST_UNROLLED, 1)]),
    "first_remainder": (HBM_N16, 0xFFFFFFFF, [(HBM_FIRST_REMAINDER, 2)]),
    "whole_unit": (HBM_N16, 0, [(1000, w) for w in range(4)]),
    # one unit in each workgroup's lanes, the lowest not in workgroup 0: 700 -> wg 2, 3500 -> wg 1, 6916 -> wg 0
    "three_units": (HBM_N16, 0, [(6916, 0), (700, 3), (3500, 1)]),
    **{f"n16_{n}": (n, 0xFFFFFFFF, [(n - 1, 2)]) for n in (1, 767, 768, 4 * 768, 4 * 768 + 1)},
}
BURN_GRID = 2
BURN_CASES = [(n, it) for n in ref.BURN_NONCES for it in ref.BURN_ITERS]
BURN_COUNTERS = [0xC0FFEE01, 0, 0xFFFFFFFF, 0x12345678]
# the kernel is told of one workgroup more than is launched: the residency wait ends at its time limit
SHORT_GRID_ID, SHORT_GRID_NONCE, SHORT_GRID_ITERS, SHORT_GRID_WAIT_TICKS = "sweep_short_grid", 0xFFFFFFFF, 4, 20000


def _live_id(n, it):
    return f"live_{n:08x}_{it}"


def _sweep_id(n, it):
    return f"sweep_{n:08x}_{it}"


def _fill_id(seed, poison):
    return f"fill_{seed:08x}_{poison}"


def _burn_id(n, it):
    return f"burn_{n:08x}_{it}"


def _requests(work: Path):
    reqs = [{"id": _live_id(n, it), "kernel": "liveness", "nonce": n, "iters": it} for n, it in LIVE_CASES]
    reqs += [{"id": _fill_id(s, p), "kernel": "hbm_fill", "n16": HBM_N16, "grid": HBM_GRID, "threads": HBM_THREADS,
              "seed": s, "poison_unit": FILL_POISONS[p]} for s, p in FILL_CASES]
    for name, (n16, seed, corrupt) in CHECK_CASES.items():
        buf = ref.hbm_pattern_words(4 * n16, seed)
        for k, (unit, word) in enumerate(corrupt):
            buf[4 * unit + word] ^= np.uint32(1 << (7 * k + 3) % 32)
        np.save(work / f"check_{name}.input.npy", buf)
        reqs.append({"id": f"check_{name}", "kernel": "hbm_check", "n16": n16, "grid": HBM_GRID,
                     "threads": HBM_THREADS, "seed": seed, "buf_npy": f"check_{name}.input.npy"})
    reqs += [{"id": _burn_id(n, it), "kernel": "burn", "nonce": n, "iters": it, "grid": BURN_GRID,
              "hbm_counters": BURN_COUNTERS} for n, it in BURN_CASES]
    # last: the 160 KiB-LDS kernel has otherwise only been dispatched through ROCr
    reqs += [{"id": _sweep_id(n, it), "kernel": "sweep", "nonce": n, "iters": it, "grid": SWEEP_GRID,
              "wait_ticks": SWEEP_WAIT_TICKS} for n, it in SWEEP_CASES]
    reqs.append({"id": SHORT_GRID_ID, "kernel": "sweep", "nonce": SHORT_GRID_NONCE, "iters": SHORT_GRID_ITERS,
                 "grid": SWEEP_GRID, "args_grid": SWEEP_GRID + 1, "wait_ticks": SHORT_GRID_WAIT_TICKS})
    return reqs


class Run:
    def __init__(self, outdir, requests, returncode, stderr):
        self.outdir, self.requests, self.returncode, self.stderr = outdir, requests, returncode, stderr

    def load(self, rid: str, name: str) -> np.ndarray:
        path = self.outdir / f"{rid}.{name}.npy"
        if not path.exists():
            pytest.fail(f"{path.name} was not written; the launcher exited {self.returncode}:\n{self.stderr[-3000:]}")
        return np.load(path)

    def canaries(self, rid: str, names) -> dict:
        return {f"{rid}.{n}": self.load(rid, f"{n}.canary") for n in names}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    work = tmp_path_factory.mktemp("raw_kernels")
    requests = _requests(work)
    (work / "requests.json").write_text(json.dumps(requests))
    outdir = work / "out"
    cmd = [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
           str(outdir)]
    try:
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
        rc, err = p.returncode, p.stderr
    except subprocess.TimeoutExpired as e:
        err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode(errors="replace")
        rc, err = "timeout", f"timed out after {e.timeout} s\n{err}"
    return Run(outdir, requests, rc, err)


BUFFERS = {"liveness": ("out", "meta", "scratch"), "sweep": ("records", "tiles", "arrive"),
           "hbm_fill": ("buf", "bad", "first_bad"), "hbm_check": ("buf", "bad", "first_bad"),
           "burn": ("records", "hbm_counters", "hbm_counters_host")}


def test_launcher_ran_every_request(run):
    assert run.returncode == 0, run.stderr[-3000:]
    status = json.loads((run.outdir / "status.json").read_text())
    assert status["error"] is None and status["completed"] == [r["id"] for r in run.requests]
    assert status["hip_library"].endswith("lib/libamdhip64.so") and "torch" not in status["hip_library"]


def test_all_canaries_intact(run):
    for req in run.requests:
        got = run.canaries(req["id"], BUFFERS[req["kernel"]])
        assert all(c.shape == (2, raw_kernels.CANARY_BYTES) for c in got.values())
        ref.check_canaries(got, raw_kernels.CANARY_FILL)


@pytest.mark.parametrize("nonce,iters", LIVE_CASES)
def test_liveness_tile_scratch_and_meta(run, nonce, iters):
    rid = _live_id(nonce, iters)
    out, scratch, meta = run.load(rid, "out"), run.load(rid, "scratch"), run.load(rid, "meta")
    assert out.dtype == np.float32 and out.size == 1024 and scratch.size == ref.SCRATCH_FLOATS
    ref.check_liveness(out.reshape(32, 32), scratch.reshape(16, 64), meta, nonce, iters)


@pytest.mark.parametrize("nonce,iters", SWEEP_CASES)
def test_chip_sweep_records_and_tiles(run, nonce, iters):
    rid = _sweep_id(nonce, iters)
    ref.check_sweep(run.load(rid, "records"), run.load(rid, "tiles"), nonce, iters, SWEEP_GRID)
    assert int(run.load(rid, "arrive")[0]) == SWEEP_GRID


@pytest.mark.parametrize("seed,poison", FILL_CASES)
def test_hbm_fill_writes_the_pattern(run, seed, poison):
    rid = _fill_id(seed, poison)
    buf = run.load(rid, "buf")
    assert buf.size == 4 * HBM_N16
    ref.check_hbm_fill(buf, HBM_N16, seed, FILL_POISONS[poison])
    if FILL_POISONS[poison] is not None:         # exactly the first word of that unit, inverted
        clean = ref.hbm_pattern_words(4 * HBM_N16, seed)
        assert np.flatnonzero(buf != clean).tolist() == [4 * FILL_POISONS[poison]]
        assert int(buf[4 * FILL_POISONS[poison]]) == int(clean[4 * FILL_POISONS[poison]]) ^ 0xFFFFFFFF
    # the fill pass leaves the check pass's counters alone
    assert int(run.load(rid, "bad")[0]) == 0 and int(run.load(rid, "first_bad")[0]) == ref.M64


@pytest.mark.parametrize("name", list(CHECK_CASES))
def test_hbm_check_counts_words_and_finds_the_first_unit(run, name):
    n16, seed, corrupt = CHECK_CASES[name]
    rid = f"check_{name}"
    ref.check_hbm_check(run.load(rid, "bad"), run.load(rid, "first_bad"), corrupt)
    # the check pass only reads the buffer
    ref.assert_bit_equal(run.load(rid, "buf"), np.load(run.outdir.parent / f"{rid}.input.npy"), "buf")


def _record_in_box(run, **figures):
    """Measured figures go to raw_kernels_box.json, in $MI355X_BOX_DIR when it is set (the
    directory a GPU run's records are collected from), else next to the arrays."""
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or run.outdir.parent)
    box_dir.mkdir(parents=True, exist_ok=True)
    path = box_dir / "raw_kernels_box.json"
    box = json.loads(path.read_text()) if path.exists() else {}
    box.update(figures)
    path.write_text(json.dumps(box, indent=1))


def test_mfma_burn_records_and_checksum(run):
    got = {(n, it): run.load(_burn_id(n, it), "records") for n, it in BURN_CASES}
    box = [{"nonce": n, "iters": it, "gpu": ref.burn_gpu_checksum(rec), "reference": ref.burn_checksum(n, it)[0],
            "bound": ref.burn_bound(it, ref.burn_checksum(n, it)[1]),
            "abs_diff_over_bound": ref.burn_ratio(rec, n, it)} for (n, it), rec in got.items()]
    _record_in_box(run, burn_margin=ref.BURN_MARGIN, burn=box)     # before anything is asserted
    print("burn |gpu - ref| / bound:", [round(b["abs_diff_over_bound"], 4) for b in box])
    for (n, it), rec in got.items():
        rid = _burn_id(n, it)
        ref.check_burn(rec, run.load(rid, "hbm_counters_host"), np.array(BURN_COUNTERS, dtype=np.uint32), n, it,
                       BURN_GRID)
        ref.assert_bit_equal(run.load(rid, "hbm_counters"), np.array(BURN_COUNTERS, dtype=np.uint32), "hbm_counters")


# ---- the same bytes through the shipped verdicts ------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.contract_cli(tmp_path_factory.mktemp("kernel_contract"))


@pytest.mark.parametrize("nonce,iters", SWEEP_CASES)
def test_sweep_verdict_on_what_the_kernel_wrote(run, cli, nonce, iters):
    rid = _sweep_id(nonce, iters)
    records, tiles = run.load(rid, "records"), run.load(rid, "tiles")
    bits = tiles.view(np.uint32)
    flipped = [(contract_cli.TILES, 2 * 1024 + 517, int(bits[2 * 1024 + 517]) ^ 1 << 22)]
    case = dict(grid=SWEEP_GRID, nonce=nonce, iters=iters)
    unknown, flip, eight = contract_cli.sweep_verdicts(
        cli, [contract_cli.sweep_case(records, tiles, num_xcc=0, variants=[flipped], **case),
              contract_cli.sweep_case(records, tiles, num_xcc=8, **case)], 3)
    print("sweep verdict:", unknown)
    ref.assert_verdict(unknown, ref.sweep_verdict(records, tiles, num_xcc=0, **case), ref.SWEEP_FLOAT_DIGITS, rid)
    # four workgroups that each hold a CU's whole LDS cannot share a CU
    assert unknown["ok"] is True and unknown["records_ok"] == 4 and unknown["cus_covered"] == 4, unknown
    assert unknown["error"] == ""
    xcc_words = {int(x) for x in records.reshape(SWEEP_GRID, 16)[:, ref.REC_XCC]}
    assert unknown["xccs_covered"] == len(xcc_words), (unknown, xcc_words)
    # four workgroups cannot cover eight XCDs
    ref.assert_verdict(eight, ref.sweep_verdict(records, tiles, num_xcc=8, **case), ref.SWEEP_FLOAT_DIGITS, rid)
    assert eight["ok"] is False and eight["records_ok"] == 4 and "/8 XCDs ran" in eight["error"], eight
    wrong = tiles.copy()
    wrong.view(np.uint32)[2 * 1024 + 517] ^= np.uint32(1 << 22)
    ref.assert_verdict(flip, ref.sweep_verdict(records, wrong, num_xcc=0, **case), ref.SWEEP_FLOAT_DIGITS, rid)
    assert flip["ok"] is False and flip["tile_bad"] == 1 and flip["records_ok"] == 3, flip


PERF_TIMES = dict(fill_us=11.3, check_us=9.7, check2_us=8.3, mfma_us=21.3)


@pytest.mark.parametrize("nonce,iters", BURN_CASES)
def test_perf_verdict_on_what_the_kernel_wrote(run, cli, nonce, iters):
    rid = _burn_id(nonce, iters)
    records = run.load(rid, "records")
    params = dict(burn_wgs=BURN_GRID, nonce=nonce, num_xcc=0, bytes=16 * HBM_N16, mfma_iters=iters, **PERF_TIMES)
    # what the check kernel counted for three corrupted units and for the last unit's last word
    found = []
    for name, bad, first in (("three_units", 3, 700), ("last_unit_word3", 1, HBM_N16 - 1)):
        counted = int(run.load(f"check_{name}", "bad")[0])
        unit = int(run.load(f"check_{name}", "first_bad")[0])
        found.append((name, bad, first, [counted, 0, unit & 0xFFFFFFFF, unit >> 32]))
    variants = [[(contract_cli.COUNTERS, i, w) for i, w in enumerate(words)] for _, _, _, words in found]
    clean = [0, 0, 0xFFFFFFFF, 0xFFFFFFFF]
    got = contract_cli.perf_verdicts(cli, [contract_cli.perf_case(records, clean, variants=variants, **params)], 3)
    print("perf verdict:", got[0])
    ref.assert_verdict(got[0], ref.perf_verdict(records, clean, **params), ref.PERF_FLOAT_DIGITS, rid)
    assert got[0]["ok"] is True and got[0]["mfma_records_ok"] == 2 and got[0]["mfma_checksum_mismatch"] == 0, got[0]
    assert got[0]["hbm_first_bad"] == -1 and got[0]["error"] == ""
    assert got[0]["clock_mhz_min"] > 0 and got[0]["clock_mhz_median"] > 0 and got[0]["clock_mhz_max"] > 0, got[0]
    for (name, bad, first, words), d in zip(found, got[1:]):
        ref.assert_verdict(d, ref.perf_verdict(records, words, **params), ref.PERF_FLOAT_DIGITS, f"{rid} {name}")
        assert d["ok"] is False and d["hbm_bad_words"] == bad and d["hbm_first_bad"] == first, (name, d)
        assert d["mfma_records_ok"] == 2 and f"hbm_bad_words={bad} first_bad_unit={first} " in d["error"], (name, d)


def test_sweep_residency_wait_ends_at_its_time_limit(run):
    """The kernel is told of SWEEP_GRID + 1 workgroups and SWEEP_GRID are launched: nobody ever
    sees the whole grid, so every workgroup leaves the wait through `elapsed > wait_ticks`, the
    exit a production sweep takes when another tenant holds a CU."""
    records, tiles = run.load(SHORT_GRID_ID, "records"), run.load(SHORT_GRID_ID, "tiles")
    recs = [[int(x) for x in row] for row in records.reshape(SWEEP_GRID, 16)]
    waited = [(r[ref.REC_T1_LO] | r[ref.REC_T1_HI] << 32) - (r[ref.REC_T0_LO] | r[ref.REC_T0_HI] << 32) for r in recs]
    arrived = [r[ref.REC_ARRIVED] for r in recs]
    _record_in_box(run, sweep_short_grid={"wait_ticks": SHORT_GRID_WAIT_TICKS, "t1_minus_t0_ticks": waited,
                                          "largest_t1_minus_t0_ticks": max(waited), "arrived": arrived})
    print("short grid: t1 - t0 ticks", waited, "arrived", arrived)
    ref.check_sweep(records, tiles, SHORT_GRID_NONCE, SHORT_GRID_ITERS, SWEEP_GRID)
    assert all(1 <= a <= SWEEP_GRID for a in arrived), arrived
    assert int(run.load(SHORT_GRID_ID, "arrive")[0]) == SWEEP_GRID
    assert all(w > SHORT_GRID_WAIT_TICKS for w in waited), waited      # straight from the loop condition
