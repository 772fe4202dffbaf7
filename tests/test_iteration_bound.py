"""MI355X_PROBE_MAX_ITERS (liveness_kernel.h): the liveness tile is "exact by
construction" only while every partial sum is an integer fp32 holds. An
exact-integer enumeration of every operand triple the generators can produce
shows that all of them are exact at the bound and that one is not one
iteration later, and every entry point that takes an iteration count keeps it
within the bound: the native prober (the daemon's -liveness_iters and the
binding's probe_iters go through it) and its Python twin, here; the probe
program and the kernel itself at the bound, in tests/test_gpu_comparators.py."""
import json
import os
import sys

import pytest

from rocm_k8s_device_plugin_amd.health import liveness
from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing.fixtures import make_mi355x_node

STUB = os.path.join(os.path.dirname(__file__), "..", "rocm_k8s_device_plugin_amd", "testing", "stub_probe.py")
BOUND = ref.PROBE_MAX_ITERS


@pytest.fixture(scope="module")
def triples():
    return ref.operand_triples()


def test_the_enumeration_reaches_every_triple(triples):
    """174 triples; the nonces near 2^32, where `i*3u + k*5u + nonce` wraps for some indices and not
    for others, reach combinations no small nonce does, the limiting one among them."""
    assert len(triples) == 174
    assert max(abs(p0 + p1) for _, p0, p1 in triples) == 12
    assert [t for t in triples if abs(t[1] + t[2]) == 12] == [(1, 6, 6)]
    small = ref.operand_triples(range(280))
    assert set(small) == set(ref.operand_triples(range(140)))   # without a wrap only nonce mod 140 counts
    assert len(small) == 112 and (1, 6, 6) not in small
    for (c, p0, p1), (n, i, j) in triples.items():              # each witness produces its triple
        assert (ref.probe_c(i, j, n), ref.probe_a(i, 0, n) * ref.probe_b(0, j, n),
                ref.probe_a(i, 1, n) * ref.probe_b(1, j, n)) == (c, p0, p1)
    n, i, j = triples[(1, 6, 6)]
    assert n > (1 << 32) - 344
    no_wrap = ((i + 2 * j + n) % 4, ((3 * i + n) % 7 - 3) * ((11 * j + n) % 5 - 2),
               ((3 * i + 5 + n) % 7 - 3) * ((11 * j + 2 + n) % 5 - 2))
    assert no_wrap != (1, 6, 6)                                  # an enumeration that forgets the wrap misses it


def test_fp32_holds_is_the_24_bit_significand():
    assert all(ref.fp32_holds(v) for v in (0, 1, -1, (1 << 24) - 1, 1 << 24, -(1 << 24), (1 << 24) + 2, 1 << 60))
    assert not any(ref.fp32_holds(v) for v in ((1 << 24) + 1, -(1 << 24) - 1, (1 << 25) + 2, 16777225, 16777219))
    import numpy as np
    for v in (16777213, 16777216, 16777217, 16777218, 16777225, 33554434, 33554436):
        assert ref.fp32_holds(v) == (int(np.float32(v)) == v), v


def test_every_partial_sum_is_exact_at_the_bound_and_one_is_not_past_it(triples):
    assert all(ref.inexact_steps(t, BOUND) == [] for t in triples)
    past = {t: ref.inexact_steps(t, BOUND + 1) for t in triples}
    assert {t for t, bad in past.items() if bad} == {(1, 6, 6)}
    # the element after both products and the host's c + float(iters) * dot, and the sum between the products
    assert sorted(set(past[(1, 6, 6)])) == [16777219, 16777225]
    # what the issue measured on the CPU: the host's formula gives 16777224, an accumulation that rounds
    # after each product 16777226
    import numpy as np
    assert int(np.float32(1) + np.float32(BOUND + 1) * np.float32(12)) == 16777224
    acc = np.float32(1 + 12 * BOUND)
    for p in (6, 6):
        acc = np.float32(acc + np.float32(p))
    assert int(acc) == 16777226
    assert BOUND == ((1 << 24) - 1) // 12


def test_the_references_bound_is_the_python_probers():
    assert liveness.PROBE_MAX_ITERS == BOUND                     # the header's: tests/test_comparator_reference.py
    assert liveness.LivenessProber(exe=STUB, iters=BOUND + 1).iters == BOUND
    assert liveness.LivenessProber(exe=STUB, iters=1 << 30).iters == BOUND
    assert liveness.LivenessProber(exe=STUB, iters=BOUND).iters == BOUND
    assert liveness.LivenessProber(exe=STUB, iters=4).iters == 4
    assert liveness.LivenessProber(exe=STUB, iters=0).iters == 1


@pytest.mark.parametrize("asked,sent", [(1 << 30, BOUND), (BOUND + 1, BOUND), (BOUND, BOUND), (4, 4), (0, 1)])
@pytest.mark.parametrize("persistent", [True, False])
def test_the_native_prober_clamps_what_it_sends_the_probe(tmp_path, asked, sent, persistent):
    """probe_iters of the binding is the daemon's -liveness_iters: both reach LivenessProber's
    configuration, and the probe program is asked for the clamped count (serve mode: the request
    line; spawn mode: --iters)."""
    from rocm_k8s_device_plugin_amd import _build
    _build.ensure_built(hip=False)
    fi = make_mi355x_node(tmp_path / "n")
    ctl, log = tmp_path / "ctl.json", tmp_path / "iters.log"
    ctl.write_text(json.dumps({}))
    eng = core().HealthEngine(str(fi.sysfs), dict(
        dev_root=str(fi.dev), liveness=True, probe_exe=STUB, argv_prefix=[sys.executable], probe_timeout_s=5.0,
        extra_env={"MI355X_STUB_PROBE_CONTROL": str(ctl), "MI355X_STUB_PROBE_ITERS_LOG": str(log)},
        probe_iters=asked, persistent=persistent))
    try:
        eng.sweep()
        assert all(ok for ok, _ in eng.snapshot().values())
    finally:
        eng.close()
    lines = log.read_text().split("\n")[:-1]
    assert lines and set(lines) == {f"probe {sent}"}, lines
