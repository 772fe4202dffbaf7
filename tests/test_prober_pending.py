"""The prober's bookkeeping between a correct reply and the verdict
(`LivenessProber::request` and `LivenessProber::check`, liveness_prober.cpp):
which nonce a late verdict is accepted against, what asks the next sweep to
restart the probe server, and when a check does not contact the server at all.

The kept-queue server keeps one outstanding dispatch per device and never
stacks a second one behind it (hsa_probe.cpp, `slot->pending`): every later
request on that device is answered pending with its own nonce, and the verdict
that comes at last carries `late` and the nonce of the first one. The stub
models just that (tests/test_gpu_prober_pending.py shows the real server doing
the same on an MI355X, and the last test here replays its recording).

What is pinned here, at engine level (`core().HealthEngine`, the stub probe):
  * a late verdict is accepted however many pending replies came before it,
    through sweeps, checks or both, and whether or not this prober saw the
    reply to the request that dispatched;
  * it is accepted against nothing else: not a nonce that was never sent, not
    one sent to a server that has been replaced;
  * a pending answer during the server's own chip sweep is no server failure;
  * a check whose budget no longer covers the request deadline sends nothing.
"""
import concurrent.futures
import json
import os
import signal
import subprocess
import sys
import threading
import time
from pathlib import Path

import pytest

from rocm_k8s_device_plugin_amd.testing.fixtures import make_mi355x_node
from rocm_k8s_device_plugin_amd.topology import discover

from test_prestart_gate import STUB, _busy_gpu, _engine, _wait_for_line

REPO = Path(__file__).resolve().parent.parent
BOX = REPO / "profiles" / "prober_pending_box.json"
HEALED_BY_SWEEP = "that a fresh process found healthy; restarting it"
HEALED_BY_CHECK = "failed a device that a fresh process found healthy (PreStartContainer check)"
DROPPED = "PreStartContainer check: probe server: probe server missed its deadline"


@pytest.fixture(scope="module", autouse=True)
def _built():
    from rocm_k8s_device_plugin_amd import _build
    _build.ensure_built(hip=False)


class _Node:
    """The engine over a fixture node and the stub, with the stub's start log
    (`log`) and its log of every line read and written (`wire`)."""

    def __init__(self, tmp_path, control=None, **opts):
        self.fi = make_mi355x_node(tmp_path / "n")
        self.inv = discover(str(self.fi.sysfs))
        self.log = tmp_path / "stub.log"
        self.wire = tmp_path / "wire.log"
        o = dict(busy_deadline_s=0.02, busy_grace_s=300.0, corroborate=False)
        o.update(opts)
        self.ctl, self.eng = _engine(self.fi, tmp_path, control or {}, env={
            "MI355X_STUB_PROBE_LOG": str(self.log), "MI355X_STUB_PROBE_REQUEST_LOG": str(self.wire)}, **o)
        self.dev = {o: d for d, o in self.eng.ordinals().items()}

    def control(self, doc):
        self.ctl.write_text(json.dumps(doc))

    def busy(self, ordinal):
        _busy_gpu(self.fi, self.inv, self.dev[ordinal])

    def starts(self):
        """The stub's start log without the "pending:<ordinal>" marks: "serve+keep" for
        a server, the ordinal for a fresh process."""
        return [ln for ln in self.log.read_text().split() if not ln.startswith("pending:")]

    def requests(self):
        return [ln[2:] for ln in self.wire.read_text().splitlines() if ln.startswith("> ")] if self.wire.exists() else []

    def replies(self, ordinal, kind="probe"):
        """What the server said of `ordinal` in its `kind` replies, in the order written."""
        out = []
        for ln in self.wire.read_text().splitlines():
            if not ln.startswith("< "):
                continue
            doc = json.loads(ln[2:])
            if doc.get("sweep") is (kind == "sweep"):
                out += [d for d in doc["devices"] if d["ordinal"] == ordinal]
        return out

    def healthy(self, ordinal):
        return self.eng.snapshot()[self.dev[ordinal]][0]

    def settled(self, check_fresh=None):
        """The conditions after a late verdict that was accepted: one server, never
        restarted, no fallback, and no fresh process ever started."""
        st = self.eng.stats()
        assert (st["server_starts"], st["server_restarts"], st["fallbacks"]) == (1, 0, 0), st
        assert self.starts() == ["serve+keep"], self.starts()
        if check_fresh is not None:
            assert st["check_fresh"] == check_fresh, st


def _late_verdict_of(node, ordinal):
    """The last probe reply for `ordinal` is the late verdict of the first request
    that found the slot clear: the scenario ran as meant."""
    said = node.replies(ordinal)
    pending = [d for d in said if d["pending_s"] > 0]
    assert said[-1]["late"] is True and said[-1]["ok"] is True, said[-1]
    assert pending and said[-1]["nonce"] == pending[0]["nonce"], (said[-1], pending[0])
    assert all(d["late"] is False for d in pending)
    return pending


# ------------------------------------------------ A1: sweeps
@pytest.mark.parametrize("n", [1, 8, 9, 12, 40, 80])
def test_late_verdict_after_n_pending_sweeps(tmp_path, n):
    """A tenant's kernel keeps device 3's dispatch queued for n sweeps; when it
    ends the late verdict carries the first sweep's nonce, and is accepted.
    (80 is past the list's own bound of 64: the oldest entry still stays.)"""
    node = _Node(tmp_path)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending"})
        for _ in range(n):
            node.eng.sweep()
            assert node.healthy(3)
        node.control({})
        node.eng.sweep()
        assert len(_late_verdict_of(node, 3)) == n
        assert node.healthy(3)
        node.settled()
        node.eng.sweep()                                  # and the slot is clear again: a plain verdict
        assert node.replies(3)[-1]["late"] is False and node.healthy(3)
        node.settled()
    finally:
        node.eng.close()


# ------------------------------------------------ A2: checks
@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("mixed", [False, True], ids=["checks", "checks_and_sweeps"])
def test_late_verdict_after_pending_checks(tmp_path, n, mixed):
    """The same with the pending replies going to PreStartContainer checks on
    the busy GPU (each inconclusive), alone or between sweeps."""
    node = _Node(tmp_path)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending"})
        for i in range(n):
            if mixed and i % 3 == 1:
                node.eng.sweep()
                continue
            r = node.eng.check([node.dev[3]], 5.0)[node.dev[3]]
            assert r["pending"] and not r["ok"], r
        node.control({})
        node.eng.sweep()
        assert len(_late_verdict_of(node, 3)) == n
        assert node.healthy(3)
        node.settled(check_fresh=0)
    finally:
        node.eng.close()


# ------------------------------------------------ A3: replies that never dispatched
def test_late_verdict_after_requests_that_never_dispatched(tmp_path):
    """One check waits out its second, longer deadline on device 3 (idle when
    it began, so the dispatch gets 40% of the budget); ten short checks meanwhile
    find the device's slot held and are answered pending without a dispatch.
    None of their nonces pushes out the one that did dispatch."""
    node = _Node(tmp_path, busy_deadline_s=0.05)
    try:
        node.eng.sweep()
        node.control({"3": "pending"})
        # budget 1.6 s: 0.05 s, then up to 0.64 s in all on the same dispatch; under 1 s is left, so no fresh process
        with concurrent.futures.ThreadPoolExecutor(11) as ex:
            long_one = ex.submit(node.eng.check, [node.dev[3]], 1.6)
            deadline = time.monotonic() + 20
            while node.log.read_text().split().count("pending:3") < 2:
                assert time.monotonic() < deadline
                time.sleep(0.005)
            node.busy(3)                                   # the tenant shows up: short deadline, inconclusive
            short = list(ex.map(lambda _: node.eng.check([node.dev[3]], 5.0)[node.dev[3]], range(10)))
            first = long_one.result()[node.dev[3]]
        assert all(r["pending"] and not r["ok"] for r in short + [first]), (short, first)
        refused = [d for d in node.replies(3) if d["error"] == "another request on this device's queue"]
        assert len(refused) >= 9, len(refused)
        node.control({})
        node.eng.sweep()
        said = node.replies(3)
        assert said[-1]["late"] is True and said[-1]["nonce"] == said[1]["nonce"], (said[1], said[-1])
        assert node.healthy(3)
        node.settled(check_fresh=0)
    finally:
        node.eng.close()


# ------------------------------------------------ A4: a dropped reply
@pytest.mark.parametrize("how", ["short_budget", "slow_reply"])
def test_late_verdict_of_a_request_whose_reply_was_dropped(tmp_path, capfd, how):
    """The check stops waiting before the server answers pending, so the prober
    never sees a reply with that nonce; the late verdict carries it all the same.
    short_budget: a budget below the busy deadline but above zero (such a check
    now sends nothing, and nothing is left on the slot). slow_reply: the budget
    covers the deadline and the server's answer comes later than the prober's
    margin for it: the line was written, the reply is dropped."""
    node = _Node(tmp_path, busy_deadline_s=0.1)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending", **({"reply_delay_s": 0.6} if how == "slow_reply" else {})})
        r = node.eng.check([node.dev[3]], 0.05 if how == "short_budget" else 5.0)[node.dev[3]]
        assert r["pending"] and not r["ok"], r
        if how == "slow_reply":
            assert DROPPED in capfd.readouterr().err
            assert node.requests()[-1].split()[-1].startswith("3:")          # the line was written ...
            deadline = time.monotonic() + 20
            while len(node.replies(3)) < 2:                                   # ... and answered, to nobody
                assert time.monotonic() < deadline
                time.sleep(0.01)
        node.control({})
        node.eng.sweep()
        if how == "slow_reply":
            _late_verdict_of(node, 3)
        assert node.healthy(3)
        node.settled(check_fresh=0)
        err = capfd.readouterr().err
        assert "stale probe result" not in err and HEALED_BY_SWEEP not in err, err
    finally:
        node.eng.close()


# ------------------------------------------------ A5: what is still refused
@pytest.mark.parametrize("mode,why", [("stale", "stale probe result"), ("fail", "differ")])
def test_a_late_verdict_that_is_wrong_still_fails_the_device(tmp_path, mode, why):
    """After 12 pending replies the late reply carries a nonce that was never
    sent (stale), or a wrong tile (fail): a definite failure, confirmed by a
    fresh process, and the device goes Unhealthy at fail_threshold (2)."""
    node = _Node(tmp_path)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending"})
        for _ in range(12):
            node.eng.sweep()
        node.control({"3": mode})
        node.eng.sweep()
        late = node.replies(3)[-1]
        sent = {int(tok.split(":")[1]) for ln in node.requests() for tok in ln.split()[4:] if tok.startswith("3:")}
        assert late["late"] is True and (late["nonce"] in sent) is (mode == "fail"), late
        assert node.starts() == ["serve+keep", "3"]                # a fresh process was asked ...
        assert node.healthy(3)                                       # ... and agreed: one failure of two
        node.eng.sweep()
        ok, reasons = node.eng.snapshot()[node.dev[3]]
        assert not ok and why in " ".join(reasons), reasons
        st = node.eng.stats()
        assert (st["server_starts"], st["server_restarts"], st["fallbacks"]) == (1, 0, 0), st
        assert all(node.healthy(o) for o in range(8) if o != 3)
    finally:
        node.eng.close()


@pytest.mark.parametrize("how", ["sigkill", "close"])
def test_nothing_from_a_replaced_server_is_accepted(tmp_path, capfd, how):
    """Three pending replies, then the server is gone (killed, or closed by the
    engine). Its successor answers late with the first of the old server's
    nonces: that is a nonce this prober did send, for this device, but not to
    this server, and the verdict is refused as stale (a fresh process is asked,
    finds the GPU healthy, and the server is restarted for it)."""
    node = _Node(tmp_path)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending"})
        for _ in range(3):
            node.eng.sweep()
        old = node.replies(3)[1]
        assert old["pending_s"] > 0
        if how == "sigkill":
            os.kill(node.eng.stats()["server_pid"], signal.SIGKILL)
            time.sleep(0.1)
        else:
            node.eng.close()
        node.control({"late_nonce": {"3": old["nonce"]}})
        node.eng.sweep()
        late = node.replies(3)[-1]
        assert late["late"] is True and late["ok"] is True and late["nonce"] == old["nonce"], late
        st = node.eng.stats()
        assert st["server_starts"] == 2 and st["server_restarts"] == 1, st
        assert node.starts() == ["serve+keep", "serve+keep", "3"], node.starts()
        err = capfd.readouterr().err
        assert "probe server failed ordinals 3 " + HEALED_BY_SWEEP in err, err
        assert node.healthy(3)
    finally:
        node.eng.close()


# ------------------------------------------------ A6: a check beside the server's own chip sweep
def test_check_during_the_servers_chip_sweep_restarts_nothing(tmp_path, capfd):
    """Every sweep is a chip sweep here, and device 4's takes 1.5 s, holding the
    device's kept slot. A check of that idle GPU meanwhile is answered pending
    twice and settled by a fresh process within its 3 s budget; a pending answer
    is no server failure, so the next sweep keeps the server."""
    node = _Node(tmp_path, chip_sweep_every=1, idle_sweeps=1, busy_deadline_s=0.05)
    try:
        node.eng.sweep()
        node.control({"4": "slow", "slow_s": 1.5})
        before = len(node.requests())
        sweep = threading.Thread(target=node.eng.sweep)
        sweep.start()
        deadline = time.monotonic() + 20
        while len(node.requests()) == before:                # the chip sweep has reached the server
            assert time.monotonic() < deadline
            time.sleep(0.005)
        assert node.requests()[-1].split()[1] == "sweep"
        t0 = time.monotonic()
        with concurrent.futures.ThreadPoolExecutor(1) as ex:
            check = ex.submit(node.eng.check, [node.dev[4]], 3.0)
            while len(node.replies(4)) < 2 and not check.done():   # both answers of the server are in:
                time.sleep(0.005)
            node.control({})                                        # the fresh process need not take 1.5 s too
            r = check.result()[node.dev[4]]
        took = time.monotonic() - t0
        sweep.join(30)
        assert not sweep.is_alive()
        assert r["ok"] and took < 3.0, (r, took)
        said = node.replies(4)
        assert len(said) == 2 and all(d["pending_s"] > 0 and d["hip_error"] == -1 for d in said), said
        assert node.eng.stats()["check_fresh"] == 1
        node.control({})
        node.eng.sweep()
        st = node.eng.stats()
        assert (st["server_starts"], st["server_restarts"]) == (1, 0), st
        err = capfd.readouterr().err
        assert HEALED_BY_CHECK not in err and HEALED_BY_SWEEP not in err, err
        assert node.healthy(4)
    finally:
        node.eng.close()


def test_definite_server_failure_a_fresh_process_contradicts_restarts_the_server(tmp_path, capfd):
    """The twin of test_definite_failure_on_a_busy_gpu_still_fails_the_check
    (test_prestart_gate.py): the server alone fails device 4 (a wrong tile from
    a stale runtime), a fresh process finds it healthy, the check passes, and
    the next sweep restarts the server."""
    node = _Node(tmp_path)
    try:
        node.eng.sweep()
        node.busy(4)
        node.control({"4": "server_fail"})
        r = node.eng.check([node.dev[4]], 5.0)[node.dev[4]]
        assert r["ok"] and not r["pending"], r
        assert node.eng.stats()["check_fresh"] == 1
        said = node.replies(4)[-1]
        assert said["ok"] is False and said["pending_s"] == 0 and said["mismatches"] > 0, said
        node.control({})
        node.eng.sweep()
        st = node.eng.stats()
        assert (st["server_starts"], st["server_restarts"]) == (2, 1), st
        assert HEALED_BY_CHECK in capfd.readouterr().err
        assert node.healthy(4)
    finally:
        node.eng.close()


# ------------------------------------------------ A7: no budget, no request
@pytest.mark.parametrize("budget", [0.0, 0.05], ids=["budget_0", "budget_below_the_deadline"])
def test_check_without_budget_for_the_deadline_sends_nothing(tmp_path, budget):
    """A check whose budget does not cover the request deadline (0.1 s here) is
    inconclusive and reaches no server: no request line, hence no dispatch left
    on the busy GPU's slot, and the next sweep's reply is a plain one."""
    node = _Node(tmp_path, busy_deadline_s=0.1)
    try:
        node.eng.sweep()
        node.busy(3)
        node.control({"3": "pending"})
        before = node.requests()
        r = node.eng.check([node.dev[3]], budget)[node.dev[3]]
        assert r["pending"] and not r["ok"], r
        idle = node.eng.check([node.dev[1]], budget)[node.dev[1]]
        assert idle["pending"] and not idle["ok"] and "check budget spent" in idle["reason"], idle
        time.sleep(0.05)
        assert node.requests() == before
        node.control({})
        node.eng.sweep()
        assert len(node.requests()) == len(before) + 1
        last = node.replies(3)[-1]
        assert last["ok"] is True and last["late"] is False, last
        assert node.healthy(3)
        node.settled(check_fresh=0)
    finally:
        node.eng.close()


# ------------------------------------------------ C3: what an MI355X said, replayed
def test_recorded_late_verdict_session_from_an_mi355x_replays_on_the_stub(tmp_path):
    """profiles/prober_pending_box.json is the raw session of
    tests/test_gpu_prober_pending.py on an MI355X: a probe at the iteration bound
    left pending by a 1 ms deadline, the pending answers after it and the late
    verdict. The same request lines to the stub in mode `slow` get the same
    (ok, late, nonce, iters, pending_s > 0, hip_error) reply by reply. The stub's
    dispatch lasts 10 times the recorded kernel time, and the replay waits that
    out before the request that got the verdict on the MI355X: a CPU's request
    round trip is not that machine's, and the order of the replies must not
    depend on it."""
    box = json.loads(BOX.read_text())
    session = box["serve"]
    late_at = [i for i, e in enumerate(session) if e["reply"]["late"]]
    assert len(late_at) == 1 and box["late"]["kernel_us"] > 1000, (late_at, box["late"])
    slow_s = 10 * box["late"]["kernel_us"] / 1e6
    ctl = tmp_path / "control.json"
    ctl.write_text(json.dumps({"0": "slow", "slow_s": slow_s}))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355X_STUB_")}
    env.pop("ROCR_VISIBLE_DEVICES", None)
    env["MI355X_STUB_PROBE_CONTROL"] = str(ctl)
    p = subprocess.Popen([sys.executable, STUB, "--serve", "--keep"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                         env=env, text=True)
    try:
        assert json.loads(p.stdout.readline())["ok"]
        what = lambda d: (d["ok"], d["late"], d["nonce"], d["iters"], d["pending_s"] > 0, d["hip_error"])  # noqa: E731
        dispatched = None
        for i, e in enumerate(session):
            if i == late_at[0]:
                assert time.monotonic() - dispatched < slow_s         # every answer so far was sure to be pending
                time.sleep(max(0.0, dispatched + slow_s + 0.05 - time.monotonic()))
            if dispatched is None and e["reply"]["pending_s"] > 0:
                dispatched = time.monotonic()
            p.stdin.write(e["request"] + "\n")
            p.stdin.flush()
            (got,) = json.loads(p.stdout.readline())["devices"]
            assert what(got) == what(e["reply"]), (e["request"], got, e["reply"])
        p.stdin.write("quit\n")
        p.stdin.flush()
        assert p.wait(timeout=30) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
