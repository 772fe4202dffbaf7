"""The real probe server's pending and late-verdict protocol on an MI355X: what
tests/test_prober_pending.py has the stub say, said by `mi355x-liveness-probe
--serve --keep`, and the shipped prober on the same path.

The one dispatch that outlives its deadline is a liveness probe at
MI355X_PROBE_MAX_ITERS: a bounded launch the suite already makes
(tests/test_gpu_comparators.py; about 37 ms, profiles/comparators_box.json)
against a 1 ms deadline. Nothing waits for longer than that kernel runs.

The raw session and the measured times are written to prober_pending_box.json
in $MI355X_BOX_DIR (default: the test's temporary directory) before anything
is asserted; profiles/prober_pending_box.json is a copy from an MI355X, which
tests/test_prober_pending.py replays against the stub on machines without a GPU.

The server has a 60 s limit of its own and is killed in any case; the engine
test starts nothing when the server did not end with status 0."""
import json
import os
import subprocess
import threading
import time
from pathlib import Path

import pytest

from test_gpu_native_health import _engine

pytestmark = pytest.mark.gpu

BOUND = 1398101          # MI355X_PROBE_MAX_ITERS (liveness_kernel.h)
SHORT = 12               # at most that many 1 ms requests behind the pending dispatch
BOX_NAME = "prober_pending_box.json"


@pytest.fixture(scope="module")
def ordinals():
    from rocm_k8s_device_plugin_amd.topology import discover, hip_ordinals
    return hip_ordinals(discover("/sys"), "/dev")


@pytest.fixture(scope="module")
def box_path(tmp_path_factory):
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or tmp_path_factory.mktemp("prober_pending"))
    box_dir.mkdir(parents=True, exist_ok=True)
    return box_dir / BOX_NAME


def _record(path, **parts):
    box = json.loads(path.read_text()) if path.exists() else {}
    box.update(parts)
    path.write_text(json.dumps(box, indent=1) + "\n")


@pytest.fixture(scope="module")
def session(ordinals, box_path):
    """One --serve --keep session: [(request line, the device's reply, ms since
    the server was ready)], the exit status, and how the requests ended."""
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    o = sorted(ordinals.values())[0]
    p = subprocess.Popen([str(probe_executable("hsa")), "--serve", "--keep"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, env=dict(os.environ, ROCR_VISIBLE_DEVICES=str(o)), text=True)
    limit = threading.Timer(60.0, p.kill)
    limit.start()
    said, ended = [], "complete"
    try:
        hello = json.loads(p.stdout.readline() or "{}")
        t0 = time.monotonic()

        def req(line):
            p.stdin.write(line + "\n")
            p.stdin.flush()
            doc = json.loads(p.stdout.readline() or "{}")
            d = (doc.get("devices") or [None])[0]
            said.append({"request": line, "reply": d, "t_ms": round((time.monotonic() - t0) * 1e3, 3)})
            return d

        def is_pending(d):
            return d is not None and not d["ok"] and d["pending_s"] > 0

        if not hello.get("ok"):
            ended = "no hello"
        elif req("probe 4 10 0:1") is None or req(f"probe {BOUND} 0.001 0:100") is None:
            ended = "no reply"
        else:
            d = said[-1]["reply"]
            for k in range(1, SHORT + 1):
                if not is_pending(d):
                    break
                d = req(f"probe 4 0.001 0:{100 + k}")
            if is_pending(d):       # the kernel outlasted all of them: this one waits for it
                d = req(f"probe 4 10 0:{100 + SHORT + 1}")
            if d is None:
                ended = "no reply"
            elif req("probe 4 10 0:200") is None:
                ended = "no reply"
        try:
            p.stdin.write("quit\n")
            p.stdin.flush()
        except OSError:
            pass
        try:
            rc = p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            rc = "timeout"
    finally:
        limit.cancel()
        if p.poll() is None:
            p.kill()
            p.wait()
    replies = [e["reply"] for e in said if e["reply"] is not None]
    pending = [d for d in replies if not d["ok"] and d["pending_s"] > 0]
    late = next((d for d in replies if d["late"]), None)
    _record(box_path, hello=hello, serve_rc=rc, ended=ended, serve=said, pending_replies=len(pending),
            pending_s=[d["pending_s"] for d in pending],
            late=None if late is None else {"kernel_us": late["kernel_us"], "total_us": late["total_us"]})
    return said, rc, ended


def test_pending_then_late_verdict_on_the_kept_queue(session):
    said, rc, ended = session
    assert ended == "complete" and rc == 0, (ended, rc, said[-1:])
    replies = [e["reply"] for e in said]
    first, dispatched, rest, after = replies[0], replies[1], replies[2:-1], replies[-1]
    assert first["ok"] and not first["late"] and first["nonce"] == 1, first
    # the dispatch at the bound outlives its 1 ms: pending, under its own nonce
    assert dispatched["ok"] is False and dispatched["pending_s"] > 0 and dispatched["hip_error"] == -1, dispatched
    assert dispatched["nonce"] == 100 and dispatched["late"] is False, dispatched
    # every request behind it is answered pending with its own nonce, until one gets the late verdict
    assert rest, said
    for e, d in zip(said[2:-2], rest[:-1]):
        want = int(e["request"].rsplit(":", 1)[1])
        assert d["ok"] is False and d["pending_s"] > 0 and d["hip_error"] == -1, d
        assert d["nonce"] == want and d["late"] is False, (e["request"], d)
    late = rest[-1]
    assert late["ok"] is True and late["late"] is True and late["nonce"] == 100 and late["iters"] == BOUND, late
    assert late["pending_s"] == 0 and late["hip_error"] == 0 and late["mismatches"] == 0, late
    # pending_s counts from the request that dispatched: it only grows
    waits = [d["pending_s"] for d in replies[1:-2]]
    assert waits == sorted(waits), waits
    # and the slot is clear again
    assert after["ok"] is True and after["late"] is False and after["nonce"] == 200 and after["iters"] == 4, after


def test_the_shipped_prober_collects_its_own_late_verdict(session, ordinals, box_path):
    """A check on an idle GPU whose first request (2 ms) leaves a real dispatch
    pending: the second request waits for that same dispatch, and its late
    verdict, under the first request's nonce, is the check's answer."""
    _, rc, ended = session
    assert ended == "complete" and rc == 0, "not started: the probe server did not end cleanly"
    dev = min(ordinals, key=ordinals.get)
    eng = _engine({dev: ordinals[dev]}, probe_iters=BOUND, busy_deadline_s=0.002)
    try:
        eng.sweep()
        swept = eng.snapshot()[dev]
        t0 = time.monotonic()
        res = eng.check([dev], 10.0)
        took = time.monotonic() - t0
        st = eng.stats()
        _record(box_path, check={"latency_ms": round(took * 1e3, 3), "result": res.get(dev),
                                 "stats": {k: st[k] for k in ("server_starts", "server_restarts", "fallbacks", "checks",
                                                              "check_fresh", "check_inconclusive")}})
        assert swept[0], swept
        assert res[dev]["ok"] and not res[dev]["pending"], res
        assert (st["check_fresh"], st["server_starts"], st["server_restarts"]) == (0, 1, 0), st
        eng.sweep()
        assert eng.snapshot()[dev][0], eng.snapshot()
        st = eng.stats()
        assert (st["server_starts"], st["server_restarts"], st["fallbacks"]) == (1, 0, 0), st
    finally:
        eng.close()
