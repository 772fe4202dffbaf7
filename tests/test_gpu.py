"""Real-hardware tests (1x MI355X via gpurun). All marked ``gpu``.

They exercise the native HIP path (no fallback exists): the in-process `_hip`
extension, the probe executable, real /sys discovery of gfx950 devices, the
HIP-ordinal <-> kfd-node mapping, amd-smi / libdrm cross-checks and one full
pod admission (fake kubelet -> plugin -> container process -> MFMA ready).
"""
import asyncio
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rocm_k8s_device_plugin_amd.ops.native import hip as load_hip
    return load_hip()


@pytest.fixture(scope="module")
def inv():
    from rocm_k8s_device_plugin_amd.topology import discover
    return discover("/sys")


@pytest.fixture(scope="module")
def ordinals(inv):
    from rocm_k8s_device_plugin_amd.topology import hip_ordinals
    return hip_ordinals(inv, "/dev")


def _location(reply):
    """(domain, kfd-style location_id) from a probe reply's dddd:bb:dd.f."""
    d, b, df = reply["pci_bus_id"].split(":")
    dev, fn = df.split(".")
    return int(d, 16), (int(b, 16) << 8) | (int(dev, 16) << 3) | int(fn, 16)


def test_inprocess_mfma_probe(hip):
    n = hip.device_count()
    assert n >= 1
    for nonce in (0, 1, 12345, 0xFFFFFFFF):
        r = hip.probe(0, nonce, 4)
        assert r["ok"], r
        assert r["mismatches"] == 0
        assert r["nonce"] == nonce
        assert r["arch"].startswith("gfx950"), r["arch"]
        assert 0 <= r["xcc_id"] < 8


def test_inprocess_probe_kernel_time_excludes_code_object_load(hip):
    """kernel_us is a warm launch; the cold one (lazy code-object load) is first_launch_us."""
    rs = [hip.probe(0, 99 + i, 4) for i in range(3)]
    assert all(r["ok"] for r in rs), rs
    # rocprof: 2.8-5 us; event pair overhead on top. The best of three: one
    # sample can carry a host-side stall between the events
    assert 0 < min(r["kernel_us"] for r in rs) < 200, rs
    for r in rs:
        if r["first_launch"]:
            assert r["first_launch_us"] > 0, r


def test_inprocess_probe_many_iters(hip):
    r = hip.probe(0, 7, 64)
    assert r["ok"] and r["iters"] == 64, r


def test_inprocess_hsa_direct_probe(hip, inv):
    """ROCr-direct path: one AQL dispatch, kfd node id straight from the agent."""
    n = hip.hsa_device_count()
    assert n >= 1
    for nonce in (3, 0xDEADBEEF):
        r = hip.hsa_probe(0, nonce, 4, 10.0)
        assert r["ok"], r
        assert r["runtime"] == "hsa" and r["dispatches"] == 1
        assert r["arch"] == "gfx950", r["arch"]
        assert r["nonce"] == nonce and r["mismatches"] == 0
        assert 0 < r["kernel_us"] < 10000
        # DRIVER_NODE_ID is the thunk's node index, which is renumbered when the
        # container's device cgroup hides GPUs; match the agent by its full PCI
        # location (kfd location_id: bus, device and function = partition index)
        assert r["kfd_node_id"] >= 0
        devs = [d for d in inv.devices if _location(r) == (d.domain, d.location_id)]
        assert len(devs) == 1, (r, inv.devices)
        assert devs[0].identity == "kfd"


@pytest.mark.parametrize("runtime", ["hsa", "hip"])
def test_probe_executable_all_devices(runtime):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    p = subprocess.run([str(probe_executable(runtime)), "--devices", "all", "--iters", "8"], capture_output=True,
                       timeout=120)
    doc = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert p.returncode == 0 and doc["ok"], doc
    assert doc["hip_device_count"] >= 1
    for d in doc["devices"]:
        assert d["ok"] and d["arch"].startswith("gfx950")
        assert d["runtime"] == runtime and d["dispatches"] == 1
        assert d["total_mem"] > 250 * 1024 ** 3  # 288 GB HBM3E per device (SPX)
    assert doc["t_ready_ns"] > doc["t_runtime_ns"] > doc["t_start_ns"]


@pytest.mark.parametrize("runtime", ["hsa", "hip"])
def test_probe_executable_bad_ordinal(runtime):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    p = subprocess.run([str(probe_executable(runtime)), "--devices", "999"], capture_output=True, timeout=120)
    assert p.returncode == 1
    doc = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert not doc["ok"]


def test_real_sysfs_discovery(inv):
    assert inv.driver_loaded and inv.kfd_present
    assert len(inv) >= 1
    # record what the real box looks like (partition strings, hive, link types)
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/real_sysfs_inventory.json", "w") as f:
        json.dump({"devices": [d.__dict__ for d in inv.devices], "partition_counts": inv.partition_counts(),
                   "compute_partition_supported": inv.compute_partition_supported(),
                   "memory_partition_supported": inv.memory_partition_supported(),
                   "kfd_nodes_readable": [n.id for n in inv.topology.nodes]}, f, indent=1, default=str)
    # kfd hides the properties of GPUs this container's device cgroup denies
    # (kfd_topology.c permission check), so only accessible GPUs carry kfd data
    readable = [d for d in inv.devices if d.identity == "kfd"]
    assert readable, "no GPU with readable kfd properties"
    gfx = {d.gfx_target_version for d in readable}
    assert gfx == {90500}, gfx
    for d in readable:
        assert d.render_minor >= 128
        assert d.numa_node >= -1
        assert d.vram_bytes > 250 * 1024 ** 3
        assert d.cu_count == 32 * d.num_xcc  # 32 CUs per XCD; SPX = 8 XCDs = 256 CUs
    assert {d.partition_type for d in inv.devices} <= {"spx_nps1", "spx_nps2", "dpx_nps1", "dpx_nps2",
                                                     "qpx_nps1", "qpx_nps2", "cpx_nps1", "cpx_nps2"}


def test_kfd_denied_gpus_identified_from_sysfs(inv, caplog):
    """The box's device cgroup denies all but the job's GPU: kfd answers EPERM
    for their topology nodes. Discovery says so (warning + metric) and still
    knows every GPU's identity and hive from PCI sysfs; for the readable GPU
    the sysfs-derived values must equal kfd's (hex unique_id -> kfd decimal)."""
    import logging
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig
    from rocm_k8s_device_plugin_amd.plugin.container import ContainerImpl
    from rocm_k8s_device_plugin_amd.topology import discover
    from rocm_k8s_device_plugin_amd.utils.metrics import REGISTRY
    kfd = [d for d in inv.devices if d.identity == "kfd"]
    assert kfd
    for d in kfd:
        dev_dir = f"/sys/bus/pci/devices/{d.bdf}"
        with open(f"{dev_dir}/unique_id") as f:
            assert str(int(f.read().strip(), 16)) == d.unique_id
        if os.path.exists(f"{dev_dir}/xgmi_hive_info/xgmi_hive_id"):
            with open(f"{dev_dir}/xgmi_hive_info/xgmi_hive_id") as f:
                assert int(f.read().strip()) == d.hive_id
    assert all(d.unique_id for d in inv.devices) and inv.placement_trusted
    if not inv.kfd_unreadable_nodes:
        pytest.skip("this box's device cgroup hides no GPU")
    assert sorted(inv.recovered) == sorted(d.id for d in inv.devices if d.identity != "kfd")
    assert any("unreadable" in w for w in inv.warnings)
    assert len({d.hive_id for d in inv.devices}) == 1      # one 8-GPU xGMI hive
    with caplog.at_level(logging.WARNING):
        impl = ContainerImpl("single", "/sys", HealthConfig(exporter_socket=None), inventory=discover("/sys"))
    assert any("kfd denies" in r.getMessage() for r in caplog.records)
    assert f"mi355x_dp_kfd_unreadable_nodes {float(len(inv.kfd_unreadable_nodes))}" in REGISTRY.render()
    from rocm_k8s_device_plugin_amd.plugin.base import new_context
    ctx = new_context("gpu")
    impl.start(ctx)
    assert impl.options(ctx).get_preferred_allocation_available
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/kfd_denied_recovery_box.json", "w") as f:
        json.dump({"kfd_unreadable_nodes": list(inv.kfd_unreadable_nodes), "recovered": inv.recovered,
                   "devices": {d.id: {"identity": d.identity, "unique_id": d.unique_id, "hive_id": str(d.hive_id),
                                      "location_id": d.location_id, "card": d.card, "render": d.render_minor}
                               for d in inv.devices},
                   "warnings": inv.warnings}, f, indent=1)


def test_hip_ordinal_mapping_matches_pci_bus(inv, ordinals, hip):
    """The ordinal we compute from kfd must be the HIP device with the same PCI location."""
    assert ordinals, "no accessible render node"
    n = hip.device_count()
    assert len(set(ordinals.values())) == n
    for dev_id, o in ordinals.items():
        d = inv.by_id[dev_id]
        ident = hip.identify(o)
        assert ident["pci_bus"] == (d.location_id >> 8) & 0xFF, (dev_id, ident, d.location_id)
        assert ident["pci_domain"] == d.domain


def test_liveness_monitor_marks_live_devices_healthy(inv, ordinals):
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig, HealthMonitor
    from rocm_k8s_device_plugin_amd.topology import Inventory
    acc = Inventory(sysfs_root="/sys", devices=tuple(inv.by_id[i] for i in ordinals), topology=inv.topology,
                    driver_loaded=True, kfd_present=True)
    mon = HealthMonitor(acc, HealthConfig(exporter_socket=None, liveness=True, liveness_timeout_s=60))
    asyncio.run(mon.check_once())
    snap = mon.snapshot()
    assert all(v.health == "Healthy" for v in snap.values()), snap


def test_probe_replies_carry_the_identity_of_their_device(inv, ordinals):
    """Every reply of the real server names the device its verdict is written
    to (full location_id), so the monitor's identity check never re-keys."""
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig, HealthMonitor
    from rocm_k8s_device_plugin_amd.topology import Inventory
    acc = Inventory(sysfs_root="/sys", devices=tuple(inv.by_id[i] for i in ordinals), topology=inv.topology,
                    driver_loaded=True, kfd_present=True)
    mon = HealthMonitor(acc, HealthConfig(exporter_socket=None, liveness=True, liveness_timeout_s=60))

    async def go():
        try:
            res = await mon.prober.probe(dict(ordinals))
            for dev_id, r in res.items():
                assert r.ok, r
                assert _location(r.detail) == (acc.by_id[dev_id].domain, acc.by_id[dev_id].location_id), \
                    (dev_id, r.detail["pci_bus_id"])
            for _ in range(3):
                await mon.check_once()
        finally:
            await mon.close()

    asyncio.run(go())
    assert mon.identity_remaps == 0 and mon.ordinals() == dict(ordinals)
    assert all(v.health == "Healthy" for v in mon.snapshot().values())


def test_corrupted_tile_turns_device_unhealthy_in_listandwatch(inv, ordinals, tmp_path, monkeypatch):
    """Fault injection on the real probe (one output bit flipped before
    verification, $MI355X_PROBE_CORRUPT_FILE re-read per request): the persistent
    server fails the tile, the fresh-process confirmation fails it too, and the
    kubelet's ListAndWatch stream shows the device Unhealthy; clearing the fault
    brings it back Healthy."""
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig
    from rocm_k8s_device_plugin_amd.plugin.container import ContainerImpl
    from rocm_k8s_device_plugin_amd.plugin.manager import ManagerConfig, PluginManager
    from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet
    from rocm_k8s_device_plugin_amd.topology import Inventory

    dev_id, o = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    acc = Inventory(sysfs_root="/sys", devices=(inv.by_id[dev_id],), topology=inv.topology,
                    driver_loaded=True, kfd_present=True)
    fault = tmp_path / "corrupt"
    fault.write_text("")
    monkeypatch.setenv("MI355X_PROBE_CORRUPT_FILE", str(fault))

    async def wait_health(k, want, timeout):
        deadline = asyncio.get_running_loop().time() + timeout
        while True:
            st = k.resources["amd.com/gpu"]
            if st.devices.get(dev_id) == want:
                return
            left = deadline - asyncio.get_running_loop().time()
            assert left > 0, f"{dev_id} never became {want}: {st.devices}"
            try:
                await k.wait_for_update("amd.com/gpu", st.updates, timeout=min(left, 2.0))
            except TimeoutError:
                pass

    async def go(tmp):
        k = FakeKubelet(tmp)
        await k.start()
        impl = ContainerImpl("single", "/sys", HealthConfig(exporter_socket=None, liveness=True,
                                                            liveness_timeout_s=30, fail_threshold=2),
                             inventory=acc)
        impl.monitor._ordinals = {dev_id: o}
        mgr = PluginManager(impl, ManagerConfig(pulse_s=0.3, plugin_dir=tmp, handle_signals=False))
        t = asyncio.create_task(mgr.run())
        try:
            await k.wait_for_resource("amd.com/gpu", 1, timeout=30)
            await wait_health(k, "Healthy", 30)
            fault.write_text("17")     # every agent: the confirming process sees this GPU as its ordinal 0
            await wait_health(k, "Unhealthy", 60)
            reasons = impl.monitor.snapshot()[dev_id].reasons
            assert any("differ" in r for r in reasons), reasons
            fault.write_text("")
            await wait_health(k, "Healthy", 60)
            assert impl.monitor.identity_remaps == 0
            assert impl.monitor.prober.server_starts >= 1
        finally:
            mgr.request_stop()
            await t
            await k.stop()

    asyncio.run(asyncio.wait_for(go(str(tmp_path)), 180))


def _probe_children(ppid):
    """PIDs of mi355x-liveness-probe processes whose parent is `ppid`."""
    out = set()
    for d in os.listdir("/proc"):
        if not d.isdigit():
            continue
        try:
            with open(f"/proc/{d}/stat") as f:
                stat = f.read()
            with open(f"/proc/{d}/cmdline", "rb") as f:
                cmd = f.read()
        except OSError:
            continue
        if int(stat.rsplit(")", 1)[1].split()[1]) == ppid and b"mi355x-liveness-probe" in cmd:
            out.add(int(d))
    return out


def test_native_daemon_corrupted_tile_reaches_listandwatch(inv, ordinals, tmp_path):
    """The same fault through the interpreter-free daemon: mi355x-device-plugin
    -liveness runs the kept-queue probe server on the real GPU; a flipped
    output bit fails the tile (server and fresh-process confirmation), the
    kubelet's ListAndWatch shows the device Unhealthy, clearing the fault
    brings it back, and SIGTERM takes the probe server down with the daemon."""
    import signal
    from rocm_k8s_device_plugin_amd.ops.native import PKG_DIR
    from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet

    # MI355X_NATIVE_DAEMON_EXE: the same test against another build (e.g. ASan/UBSan, host code only);
    # the probe server is always this tree's gfx950 build
    exe = os.environ.get("MI355X_NATIVE_DAEMON_EXE") or os.path.join(str(PKG_DIR), "bin", "mi355x-device-plugin")
    probe = os.path.join(str(PKG_DIR), "bin", "mi355x-liveness-probe")
    dev_id, o = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    fault = tmp_path / "corrupt"
    fault.write_text("")
    kdir = str(tmp_path / "dp")

    async def wait_health(k, want, timeout):
        deadline = asyncio.get_running_loop().time() + timeout
        while True:
            st = k.resources["amd.com/gpu"]
            if st.devices.get(dev_id) == want:
                return
            left = deadline - asyncio.get_running_loop().time()
            assert left > 0, f"{dev_id} never became {want}: {st.devices}"
            try:
                await k.wait_for_update("amd.com/gpu", st.updates, timeout=min(left, 2.0))
            except TimeoutError:
                pass

    import socket
    import urllib.request
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]

    def metrics():
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/metrics", timeout=5) as r:
            return {k: float(v) for k, v in (ln.rsplit(" ", 1) for ln in r.read().decode().splitlines()
                                             if ln and not ln.startswith("#"))}

    async def go():
        k = FakeKubelet(kdir)
        await k.start()
        env = dict(os.environ, MI355X_PROBE_CORRUPT_FILE=str(fault))
        proc = await asyncio.create_subprocess_exec(
            exe, "-kubelet_dir", kdir, "-exporter_socket", "", "-pulse", "1", "-liveness", "-liveness_probe", probe,
            "-liveness_timeout", "30",
            "-liveness_fail_threshold", "2", "-metrics_port", str(port), "-device_list_strategy",
            "device-specs,cdi-cri", "-cdi_spec_dir", str(tmp_path / "cdi"), stdout=asyncio.subprocess.DEVNULL,
            stderr=asyncio.subprocess.PIPE, env=env)
        try:
            await k.wait_for_resource("amd.com/gpu", 1, timeout=60)
            await wait_health(k, "Healthy", 60)
            children.update(_probe_children(proc.pid))
            assert children, "no probe server under the daemon"
            # CDI names next to the DeviceSpecs, the spec file on disk
            adm = await k.admit("amd.com/gpu", 1, must_include=[dev_id])
            car = adm.response.container_responses[0]
            assert [c.name for c in car.cdi_devices] == [f"amd.com/gpu={dev_id}"] and car.devices
            assert (tmp_path / "cdi" / "amd.com-gpu.json").exists()
            k.release("amd.com/gpu", adm.device_ids)
            m = await asyncio.to_thread(metrics)
            assert m[f'mi355x_dp_device_healthy{{device="{dev_id}"}}'] == 1.0
            assert m[f'mi355x_dp_liveness_probe_ms{{device="{dev_id}"}}'] > 0
            # the real kept-queue server's own kfd entry is found: busy state is known
            assert m["mi355x_dp_busy_state_known"] == 1.0
            fault.write_text("17")
            await wait_health(k, "Unhealthy", 60)
            m = await asyncio.to_thread(metrics)
            assert m[f'mi355x_dp_device_healthy{{device="{dev_id}"}}'] == 0.0
            fault.write_text("")
            await wait_health(k, "Healthy", 60)
        finally:
            if proc.returncode is None:
                proc.send_signal(signal.SIGTERM)
            _, err = await asyncio.wait_for(proc.communicate(), 30)
            print(err.decode(errors="replace")[-4000:])   # the daemon's log, shown when the test fails
            await k.stop()
        err = err.decode(errors="replace")
        assert proc.returncode == 0, err[-3000:]
        assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "ThreadSanitizer" not in err, err[-3000:]
        assert f"device {dev_id}: Healthy -> Unhealthy liveness probe:" in err and "differ" in err, err[-3000:]
        return err

    children = set()
    asyncio.run(asyncio.wait_for(go(), 240))
    # the daemon's probe server went down with it
    assert not [pid for pid in children if os.path.exists(f"/proc/{pid}")], children


def test_native_daemon_prestart_gate(ordinals, tmp_path):
    """-prestart_liveness on MI355X: kubelet's PreStartContainer probes the
    pod's GPU through the daemon's kept-queue probe server right before the
    container starts. A healthy GPU passes in about a millisecond; a flipped
    output bit fails the start with FAILED_PRECONDITION naming the device."""
    import signal
    import time
    from rocm_k8s_device_plugin_amd.ops.native import PKG_DIR
    from rocm_k8s_device_plugin_amd.proto import deviceplugin as pb
    from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet, NativeRpcError

    exe = os.environ.get("MI355X_NATIVE_DAEMON_EXE") or os.path.join(str(PKG_DIR), "bin", "mi355x-device-plugin")
    probe = os.path.join(str(PKG_DIR), "bin", "mi355x-liveness-probe")
    dev_id, _ = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    fault = tmp_path / "corrupt"
    fault.write_text("")
    kdir = str(tmp_path / "dp")
    out = {}

    async def go():
        k = FakeKubelet(kdir, rpc_client="native")
        await k.start()
        env = dict(os.environ, MI355X_PROBE_CORRUPT_FILE=str(fault))
        proc = await asyncio.create_subprocess_exec(
            exe, "-kubelet_dir", kdir, "-exporter_socket", "", "-pulse", "3600", "-liveness", "-liveness_probe",
            probe, "-liveness_timeout", "30", "-prestart_liveness", stdout=asyncio.subprocess.DEVNULL,
            stderr=asyncio.subprocess.PIPE, env=env)
        try:
            st = await k.wait_for_resource("amd.com/gpu", 1, timeout=60)
            assert st.options.pre_start_required and st.devices.get(dev_id) == "Healthy"
            adm = await k.admit("amd.com/gpu", 1, must_include=[dev_id])
            assert adm.prestart_ms > 0
            k.release("amd.com/gpu", adm.device_ids)
            req = pb.PreStartContainerRequest(devices_ids=[dev_id])
            lat = []
            for _ in range(20):
                t0 = time.perf_counter()
                await k._call(st, "PreStartContainer", req, pb.PreStartContainerResponse, timeout=30.0)
                lat.append((time.perf_counter() - t0) * 1e3)
            lat.sort()
            out["prestart_ms_p50"], out["prestart_ms_max"] = lat[len(lat) // 2], lat[-1]
            assert out["prestart_ms_p50"] < 50, lat
            fault.write_text("17")
            with pytest.raises(NativeRpcError) as e:
                await k._call(st, "PreStartContainer", req, pb.PreStartContainerResponse, timeout=30.0)
            assert e.value.status == 9 and dev_id in e.value.message and "differ" in e.value.message, e.value.message
            fault.write_text("")
            await k._call(st, "PreStartContainer", req, pb.PreStartContainerResponse, timeout=30.0)
        finally:
            if proc.returncode is None:
                proc.send_signal(signal.SIGTERM)
            _, err = await asyncio.wait_for(proc.communicate(), 30)
            print(err.decode(errors="replace")[-3000:])
            await k.stop()
        err = err.decode(errors="replace")
        assert proc.returncode == 0, err[-3000:]
        assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "ThreadSanitizer" not in err

    asyncio.run(asyncio.wait_for(go(), 240))
    print(f"prestart gate on {dev_id}: p50 {out['prestart_ms_p50']:.2f} ms, max {out['prestart_ms_max']:.2f} ms")
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/prestart_gate_box.json", "w") as f:
        json.dump({"device": dev_id, **out}, f)


def _foreign_queue_pids(gpu_id, exclude=()):
    """kfd proc entries (host PIDs) other than `exclude` with a user queue on kfd gpu_id."""
    root = "/sys/class/kfd/kfd/proc"
    out = set()
    for pid in os.listdir(root) if os.path.isdir(root) else []:
        if not pid.isdigit() or int(pid) in exclude:
            continue
        qdir = os.path.join(root, pid, "queues")
        try:
            for q in os.listdir(qdir):
                with open(os.path.join(qdir, q, "gpuid")) as f:
                    if int(f.read().strip() or 0) == gpu_id:
                        out.add(int(pid))
        except OSError:
            continue
    return out


def test_native_daemon_chip_sweep_and_throughput_check(inv, ordinals, tmp_path):
    """mi355x-device-plugin runs the full-chip sweep and the throughput check
    through its kept-queue probe server on the real GPU; the rates reach
    /metrics and the device stays Healthy."""
    import signal
    import socket
    import urllib.request
    from rocm_k8s_device_plugin_amd.ops.native import PKG_DIR
    from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet

    # MI355X_NATIVE_DAEMON_EXE: the same test against another build (e.g. ASan/UBSan, host code only);
    # the probe server is always this tree's gfx950 build
    exe = os.environ.get("MI355X_NATIVE_DAEMON_EXE") or os.path.join(str(PKG_DIR), "bin", "mi355x-device-plugin")
    probe = os.path.join(str(PKG_DIR), "bin", "mi355x-liveness-probe")
    dev_id = sorted(ordinals.items(), key=lambda kv: kv[1])[0][0]
    gpu_id = inv.topology.node(inv.by_id[dev_id].node_id).gpu_id
    kdir = str(tmp_path / "dp")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]

    def metrics():
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/metrics", timeout=5) as r:
            return {k: float(v) for k, v in (ln.rsplit(" ", 1) for ln in r.read().decode().splitlines()
                                             if ln and not ln.startswith("#"))}

    # processes that already hold queues on this GPU (kfd names them by host PID; e.g. this pytest
    # process after the in-process HIP tests): then the daemon must leave the GPU alone
    busy = bool(_foreign_queue_pids(gpu_id))

    async def go():
        k = FakeKubelet(kdir)
        await k.start()
        proc = await asyncio.create_subprocess_exec(
            exe, "-kubelet_dir", kdir, "-exporter_socket", "", "-pulse", "1", "-liveness", "-liveness_probe", probe,
            "-liveness_timeout", "30",
            "-liveness_chip_sweep_every", "2", "-perf_check_every", "3", "-perf_mib", "1024",
            "-metrics_port", str(port), stdout=asyncio.subprocess.DEVNULL, stderr=asyncio.subprocess.PIPE)
        try:
            st = await k.wait_for_resource("amd.com/gpu", 1, timeout=60)
            m = {}
            for _ in range(120):
                m = await asyncio.to_thread(metrics)
                if m.get("mi355x_dp_chip_sweeps_total", 0) >= 2 and m.get("mi355x_dp_perf_checks_total", 0) >= 1:
                    break
                if busy and m.get("mi355x_dp_liveness_probe_ms{device=\"%s\"}" % dev_id, 0) > 0:
                    break
                await asyncio.sleep(0.5)
            if busy:
                await asyncio.sleep(3.5)   # a few more pulses: still no sweep, no throughput check
                m = await asyncio.to_thread(metrics)
                assert m.get("mi355x_dp_chip_sweeps_total", 0) == 0, m
                assert f'mi355x_dp_perf_state{{device="{dev_id}"}}' not in m, m
            else:
                assert m.get("mi355x_dp_chip_sweeps_total", 0) >= 2, m
                assert m[f'mi355x_dp_perf_state{{device="{dev_id}"}}'] == 0.0, m
                # plausible MI355X rates (HBM3E peak 8 TB/s, dense bf16 2.5 PFLOP/s): broken dispatch
                # timing (e.g. under a kernel-tracing profiler) shows as absurd values
                assert 1000 < m[f'mi355x_dp_perf_hbm_read_gbps{{device="{dev_id}"}}'] < 9000, m
                assert 500 < m[f'mi355x_dp_perf_mfma_tflops{{device="{dev_id}"}}'] < 2600, m
            assert k.resources["amd.com/gpu"].devices[dev_id] == "Healthy"
        finally:
            if proc.returncode is None:
                proc.send_signal(signal.SIGTERM)
            _, err = await asyncio.wait_for(proc.communicate(), 30)
            print(err.decode(errors="replace")[-4000:])   # the daemon's log, shown when the test fails
            await k.stop()
        err = err.decode(errors="replace")
        assert proc.returncode == 0, err[-3000:]
        assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "ThreadSanitizer" not in err, err[-3000:]
        return m

    m = asyncio.run(asyncio.wait_for(go(), 240))
    print(json.dumps({k: v for k, v in m.items() if "perf" in k or "chip" in k}))


def test_probe_cli_corrupt_word_fails_the_tile():
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    p = subprocess.run([str(probe_executable("hsa")), "--devices", "0", "--corrupt-word", "3"], capture_output=True,
                       timeout=120)
    doc = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert p.returncode == 1 and not doc["ok"], doc
    d = doc["devices"][0]
    assert d["mismatches"] == 1 and d["hip_error"] == 0, d


def test_persistent_probe_server(ordinals):
    """One --serve process answers several sweeps; per-sweep cost is device work only."""
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    prober = LivenessProber(timeout_s=60, mode="persistent")
    ords = dict(ordinals)

    async def go():
        lat = []
        for _ in range(4):
            res = await prober.probe(ords)
            assert all(r.ok for r in res.values()), res
            assert all(r.detail["runtime"] == "hsa" and r.detail["dispatches"] == 1 for r in res.values())
            lat.append(max(r.latency_ms for r in res.values()))
        assert prober.server_starts == 1 and prober.fallbacks == 0
        await prober.close()
        return lat

    lat = asyncio.run(go())
    # the first sweep includes ROCr start-up; later sweeps only code object + queue + dispatch
    assert min(lat[1:]) < 100.0, lat


def test_persistent_probe_server_keeps_queues(ordinals):
    """--serve --keep: the first sweep sets the device up, later sweeps are one packet each (no set-up, fresh
    nonce verified every time); a kept device survives many sweeps."""
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    prober = LivenessProber(timeout_s=60, mode="persistent", keep_queues=True)
    ords = dict(ordinals)

    async def go():
        docs = []
        for _ in range(12):
            res = await prober.probe(ords)
            assert all(r.ok for r in res.values()), res
            docs.append([r.detail for r in res.values()])
        assert prober.server_starts == 1 and prober.fallbacks == 0
        await prober.close()
        return docs

    docs = asyncio.run(go())
    assert all(d["setup_us"] > 1000 for d in docs[0])        # queue + executable on the first sweep
    for sweep in docs[1:]:
        for d in sweep:
            assert d["setup_us"] == 0 and d["dispatches"] == 1 and d["mismatches"] == 0
    # one AQL packet + wait, no kfd ioctls: the median sweep (a single one can be descheduled)
    import statistics
    assert statistics.median(d["total_us"] for sweep in docs[1:] for d in sweep) < 5000, docs
    assert len({d["nonce"] for sweep in docs for d in sweep}) == sum(len(s) for s in docs)


def test_kept_queue_server_is_not_a_tenant(inv, ordinals):
    """The kept-queue server's own kfd entry is found and excluded: its queue does not make the GPU look busy."""
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    from rocm_k8s_device_plugin_amd.topology import kfd_busy_gpu_ids
    dev_id, o = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    gid = inv.topology.node(inv.by_id[dev_id].node_id).gpu_id
    prober = LivenessProber(timeout_s=60, mode="persistent", keep_queues=True)

    async def go():
        before = kfd_busy_gpu_ids("/sys")     # this test process may hold HIP queues of its own
        res = await prober.probe({dev_id: o})
        assert all(r.ok for r in res.values()), res
        # on the shared host another tenant's GPU process may have started in the
        # same instant as the server: queue coverage of our GPU resolves it, else
        # the claim stays empty (the safe side) until the other one exits
        own = prober.own_kfd_entries_for({gid})
        for _ in range(100):
            if own:
                break
            await asyncio.sleep(0.1)
            own = prober.own_kfd_entries_for({gid})
        if not own:
            await prober.close()
            pytest.skip(f"another GPU process started with the probe server and is still running: "
                        f"{sorted(prober._own_kfd)}")
        assert len(own) == 1, own
        qdir = os.path.join("/sys/class/kfd/kfd/proc", next(iter(own)), "queues")
        gids = {int(open(os.path.join(qdir, q, "gpuid")).read()) for q in os.listdir(qdir)}
        assert gid in gids                                          # the server's kept queue
        # ... is not counted as a tenant (other GPUs of the shared host come and go: look at ours only)
        assert (gid in kfd_busy_gpu_ids("/sys", exclude=own)) == (gid in before)
        await prober.close()

    asyncio.run(go())


def test_peer_probe_self_copy(ordinals):
    """H2 path on one GPU: HBM -> HBM DMA copy, readback, word-exact verify."""
    from rocm_k8s_device_plugin_amd.health.peer import probe_peers
    o = sorted(ordinals.values())[0]
    rep = probe_peers([o], nbytes=32 << 20, reps=3, timeout_s=120)
    assert rep.ok, rep
    (p,) = rep.pairs
    assert p["src"] == p["dst"] == o and p["mismatches"] == 0 and p["bytes"] == 32 << 20
    assert p["gbps_best"] > 10.0, p           # an HBM-local DMA copy on MI355X
    assert rep.summary()["pairs_ok"] == 1


def test_peer_probe_xgmi_pair(ordinals):
    """H2 over a real link: on a box with 2+ accessible MI355X GPUs (the 1-GPU
    test box has one: skipped), every ordered pair is copied and verified over
    xGMI, one hop."""
    from rocm_k8s_device_plugin_amd.health.peer import probe_peers
    ords = sorted(ordinals.values())
    if len(ords) < 2:
        pytest.skip("one accessible GPU")
    rep = probe_peers(ords[:2], nbytes=32 << 20, reps=3, timeout_s=120)
    assert rep.ok, rep
    cross = [p for p in rep.pairs if p["src"] != p["dst"]]
    assert len(cross) == 2 and all(p["mismatches"] == 0 for p in cross), cross
    assert rep.summary()["link_types"] == ["xgmi"], rep.summary()


def test_smi_event_watcher_subscribes(inv):
    """amd-smi event notification starts on the real GPU and drains without error.

    A liveness probe run while subscribed makes kfd emit nothing we subscribe
    to (no reset/fault), so the expectation is an empty or benign list."""
    from rocm_k8s_device_plugin_amd.ops.native import core
    w = core().SmiEventWatcher()
    mask = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 3) | (1 << 8)
    err = w.start(mask)
    assert err == "", err
    assert w.running and w.devices >= 1
    ev = w.poll(50)
    assert all(e["name"] in ("vmfault", "thermal_throttle", "gpu_pre_reset", "gpu_post_reset", "queue_eviction")
               for e in ev), ev
    w.stop()
    assert not w.running
    assert w.poll(0) == []


def test_container_with_node_view_mounts(tmp_path, inv, ordinals):
    """The fake runtime applies -node_view mounts (by redirection) and ROCr in the
    container skips the host's per-CPU cache walk, with the same MFMA verdict.

    Asserted is the mechanism, which is deterministic: the viewed container
    opens no cache descriptor under the node tree and issues at least one read
    syscall fewer per hidden directory. Both containers run the same
    interposing build with the same /dev view. The wall-clock hsa_init of one
    sample each is only reported: on a shared host it follows other tenants'
    kfd and sysfs traffic (round 4's driver box: 105 ms viewed vs 48 ms plain)."""
    from rocm_k8s_device_plugin_amd.container_runtime import start_container, wait_kfd_released
    from rocm_k8s_device_plugin_amd.node_view import NodeView
    dev_id, o = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    paths = ["/dev/kfd"] + inv.by_id[dev_id].dev_paths()
    nv = NodeView(str(tmp_path / "nv"), "/sys", alias="/sys/devices/system/node")
    mounts = [(ctr, host) for host, ctr in nv.mounts()]
    plain = start_container([o], timeout_s=120, device_paths=paths)
    assert plain.ok, plain.error
    wait_kfd_released(plain.kfd_lingering)
    viewed = start_container([o], timeout_s=120, device_paths=paths, mounts=mounts)
    assert viewed.ok, viewed.error
    wait_kfd_released(viewed.kfd_lingering)
    assert viewed.doc["devices"][0]["mismatches"] == 0
    keys = ("hsa_init_us", "read_syscalls_runtime", "cpu_ms_runtime", "view")
    row = lambda r: dict(zip(keys, (r.doc["init_us"]["hsa_init"], r.doc["read_syscalls_runtime"],
                                    r.doc["cpu_ms_runtime"], r.doc["view"])))
    rep = {"hidden_cache_dirs": nv.hidden, "plain": row(plain), "viewed": row(viewed)}
    print(json.dumps(rep))
    assert nv.hidden > 0, rep
    assert viewed.doc["view"]["redirected"] > 0, rep
    assert viewed.doc["view"]["node_cpu_cache_opens"] == 0, rep
    if plain.doc["view"]["node_cpu_cache_opens"] == 0:
        pytest.skip(f"this host's ROCr walks no per-CPU cache descriptor: nothing for the view to save ({rep})")
    saved = plain.doc["read_syscalls_runtime"] - viewed.doc["read_syscalls_runtime"]
    assert saved >= nv.hidden, rep


@pytest.mark.parametrize("runtime", ["hsa", "hip"])
def test_container_dev_view_hides_unallocated_gpus(inv, ordinals, runtime):
    """The fake runtime's /dev view is what ROCr sees: with the GPU's render node
    in the DeviceSpecs the container runs on it; handed a node the test process
    cannot open (another tenant's GPU on a 1-GPU box) the thunk finds no GPU
    and the container does not become ready; handed another GPU the process can
    open (a multi-GPU box) it runs on exactly that one."""
    from rocm_k8s_device_plugin_amd.container_runtime import start_container, wait_kfd_released
    dev_id, o = sorted(ordinals.items(), key=lambda kv: kv[1])[0]
    g = inv.by_id[dev_id]
    ok = start_container([o], timeout_s=120, device_paths=["/dev/kfd"] + g.dev_paths(), runtime=runtime)
    assert ok.ok, ok.error
    assert ok.doc["hip_device_count"] == 1
    assert ok.doc["devices"][0]["pci_bus_id"].lower() == dev_id.lower()
    wait_kfd_released(ok.kfd_lingering)
    others = [d for d in inv.devices if d.render_minor >= 0 and d.render_minor != g.render_minor]
    hidden = [d for d in others if d.id not in ordinals]       # render node not openable here
    wrong = ["/dev/kfd"] + (hidden[0].dev_paths() if hidden else ["/dev/dri/renderD1"])
    bad = start_container([o], timeout_s=120, device_paths=wrong, runtime=runtime)
    wait_kfd_released(bad.kfd_lingering)
    assert not bad.ok
    assert bad.doc.get("hip_device_count", 0) == 0, bad.doc
    reachable = [d for d in others if d.id in ordinals]
    if reachable:
        h = reachable[0]
        r = start_container([ordinals[h.id]], timeout_s=120, device_paths=["/dev/kfd"] + h.dev_paths(),
                            runtime=runtime)
        wait_kfd_released(r.kfd_lingering)
        assert r.ok and r.doc["hip_device_count"] == 1, r.error
        assert r.doc["devices"][0]["pci_bus_id"].lower() == h.id.lower()


def test_chip_sweep_covers_every_cu_and_xcd(ordinals):
    """Full-chip sweep: one workgroup per CU, all resident together, every XCD runs
    and every MFMA tile / LDS word is exact (one-shot and through the server)."""
    import json
    import subprocess
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    o = sorted(ordinals.values())[0]
    env = dict(os.environ, ROCR_VISIBLE_DEVICES=str(o))
    p = subprocess.run([str(probe_executable("hsa")), "--sweep", "--devices", "0", "--timeout", "20"],
                       stdout=subprocess.PIPE, env=env, timeout=120)
    d = json.loads(p.stdout.decode().strip().splitlines()[-1])["devices"][0]
    assert p.returncode == 0 and d["ok"], d
    assert d["grid"] == d["cu_count"] == d["cus_covered"], d
    assert d["num_xcc"] == d["xccs_covered"] == 8 and len(set(d["wgs_per_xcc"])) == 1, d
    assert d["mfma_bad"] == d["lds_bad"] == d["tile_bad"] == 0 and d["all_resident"], d
    prober = LivenessProber(timeout_s=60)

    async def go():
        res = await prober.sweep({"gpu": o})
        await prober.close()
        return res["gpu"]

    r = asyncio.run(go())
    assert r.ok and r.detail["cus_covered"] == r.detail["cu_count"], r


def test_perf_check_measures_hbm_and_mfma(ordinals):
    """Throughput check on the real GPU: the HBM pattern reads back exact, every
    XCD runs MFMA workgroups with identical checksums, and the rates are those
    of a healthy MI355X (well above the monitor's default floors)."""
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    o = sorted(ordinals.values())[0]
    env = dict(os.environ, ROCR_VISIBLE_DEVICES=str(o))
    p = subprocess.run([str(probe_executable("hsa")), "--perf", "--perf-mib", "2048", "--perf-iters", "32768",
                        "--devices", "0", "--timeout", "20"], stdout=subprocess.PIPE, env=env, timeout=120)
    d = json.loads(p.stdout.decode().strip().splitlines()[-1])["devices"][0]
    assert p.returncode == 0 and d["ok"], d
    assert d["hbm_bad_words"] == 0 and d["hbm_first_bad"] == -1 and d["mfma_checksum_mismatch"] == 0, d
    assert d["mfma_records_ok"] == d["mfma_grid"] == 2 * d["cu_count"] and d["mfma_xccs"] == d["num_xcc"] == 8, d
    floors = HealthConfig()
    assert d["hbm_read_gbps"] > floors.perf_min_hbm_read_gbps, d
    assert d["hbm_write_gbps"] > floors.perf_min_hbm_write_gbps, d
    assert d["mfma_tflops"] > floors.perf_min_mfma_tflops, d
    assert all(500 < c < 2500 for c in d["xcd_clock_mhz"]), d
    # the monitor's path: the persistent server's "perf" request
    prober = LivenessProber(timeout_s=60)
    prober.perf_mib, prober.perf_iters = 1024, 16384

    async def go():
        res = await prober.perf({"gpu": o})
        await prober.close()
        return res["gpu"]

    r = asyncio.run(go())
    assert r.ok and r.detail["hbm_bad_words"] == 0 and r.detail["mfma_xccs"] == 8, r


def test_perf_check_finds_an_injected_hbm_fault(ordinals):
    """--poison-hbm U: the fill writes unit U with one word inverted; the check
    pass must count exactly that word and name that unit."""
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    o = sorted(ordinals.values())[0]
    env = dict(os.environ, ROCR_VISIBLE_DEVICES=str(o))
    unit = 12_345_677
    p = subprocess.run([str(probe_executable("hsa")), "--perf", "--perf-mib", "512", "--perf-iters", "1024",
                        "--poison-hbm", str(unit), "--devices", "0", "--timeout", "20"], stdout=subprocess.PIPE,
                       env=env, timeout=120)
    d = json.loads(p.stdout.decode().strip().splitlines()[-1])["devices"][0]
    assert p.returncode == 1 and not d["ok"], d
    assert d["hbm_bad_words"] == 1 and d["hbm_first_bad"] == unit and d["mfma_checksum_mismatch"] == 0, d
    assert "hbm_bad_words=1" in d["error"], d


def test_sweep_and_perf_check_borrow_the_kept_queue(ordinals):
    """With kept queues the chip sweep and the throughput check run on the
    device's kept probe queue (set up by whichever comes first), so the probe
    server holds two 181 MB save areas per GPU (its queue, ROCr's internal
    one), not three; probes before and after still verify fresh nonces."""
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    o = sorted(ordinals.values())[0]
    prober = LivenessProber(timeout_s=60)
    prober.perf_mib, prober.perf_iters = 1024, 8192

    async def go():
        sw = (await prober.sweep({"gpu": o}))["gpu"]      # first request: sets the kept slot up
        pr = (await prober.probe({"gpu": o}))["gpu"]
        pf = (await prober.perf({"gpu": o}))["gpu"]
        sw2 = (await prober.sweep({"gpu": o}))["gpu"]
        pr2 = (await prober.probe({"gpu": o}))["gpu"]
        with open(f"/proc/{prober._server.proc.pid}/status") as f:
            rss_mb = [int(line.split()[1]) for line in f if line.startswith("VmRSS")][0] / 1024
        await prober.close()
        return sw, pr, pf, sw2, pr2, rss_mb

    sw, pr, pf, sw2, pr2, rss_mb = asyncio.run(go())
    assert sw.ok and sw2.ok and pf.ok and pr.ok and pr2.ok, (sw, pr, pf, sw2, pr2)
    assert sw.detail["kept_queue"] and sw2.detail["kept_queue"] and pf.detail["kept_queue"], (sw, pf, sw2)
    assert rss_mb < 450, rss_mb


def test_probe_server_killed_between_sweeps_is_replaced(ordinals):
    """SIGKILL of the real probe server (OOM killer, operator): the next sweep
    starts a new one and verifies a fresh nonce; no verdict is lost."""
    import signal as _signal
    from rocm_k8s_device_plugin_amd.health.liveness import LivenessProber
    o = sorted(ordinals.values())[0]
    prober = LivenessProber(timeout_s=60)

    async def go():
        first = (await prober.probe({"gpu": o}))["gpu"]
        os.kill(prober._server.proc.pid, _signal.SIGKILL)
        await asyncio.sleep(0.5)
        second = (await prober.probe({"gpu": o}))["gpu"]
        starts = prober.server_starts
        await prober.close()
        return first, second, starts

    first, second, starts = asyncio.run(go())
    assert first.ok and second.ok, (first, second)
    assert starts == 2 and second.detail["nonce"] != first.detail["nonce"]


def test_check_past_its_deadline_on_the_kept_queue(ordinals):
    """The abandon path on hardware, without a hang: a throughput check whose
    MFMA burn (~0.3 s here) outlives a 1 us deadline is reported in flight (its
    signal and buffers go to the in-flight registry, the kept queue is marked
    blocked; a probe meanwhile reports pending); once the kernel has finished,
    probes, sweeps and checks on that GPU run normally again."""
    import time
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    o = sorted(ordinals.values())[0]
    env = dict(os.environ, ROCR_VISIBLE_DEVICES=str(o))
    p = subprocess.Popen([str(probe_executable("hsa")), "--serve", "--keep"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, env=env, text=True)
    try:
        assert json.loads(p.stdout.readline())["ok"]

        def req(line):
            p.stdin.write(line + "\n")
            p.stdin.flush()
            return json.loads(p.stdout.readline())

        assert req("probe 4 10 0:1")["devices"][0]["ok"]                 # sets the kept slot up
        late = req("perf 4194304 0.000001 64 0:2")["devices"][0]          # burn >> the 1 us deadline
        assert not late["ok"] and late["hsa_error"] == -1 and late["kept_queue"], late
        assert "MFMA burn did not complete" in late["error"], late
        blocked = req("probe 4 0.05 0:3")["devices"][0]                   # queued behind the burn
        assert not blocked["ok"] and blocked["pending_s"] > 0, blocked
        time.sleep(1.0)                                                   # the burn has finished
        after = req("probe 4 10 0:4")["devices"][0]
        assert after["ok"] and after["nonce"] == 4, after
        sweep = req("sweep 4 10 0:5")["devices"][0]
        assert sweep["ok"] and sweep["kept_queue"], sweep
        perf = req("perf 1024 10 64 0:6")["devices"][0]
        assert perf["ok"] and perf["kept_queue"] and perf["hbm_bad_words"] == 0, perf
        p.stdin.write("quit\n")
        p.stdin.flush()
        assert p.wait(timeout=30) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()


_CHECK_FLAGS = {
    "sweep": ["--sweep", "--iters", "1"],
    "perf": ["--perf", "--perf-mib", "64", "--perf-iters", "1024"],     # 64 MiB: the smallest buffer accepted
    "datapath": ["--datapath"],
}
# what a reply that never reached a device must leave at zero
_CHECK_COUNTERS = {
    "sweep": ["hsa_error", "iters", "grid", "cu_count", "num_xcc", "records_ok", "mfma_bad", "lds_bad",
              "tile_bad", "cus_covered", "xccs_covered", "kernel_us", "arrival_spread_us", "total_us", "in_flight_s"],
    "perf": ["hsa_error", "bytes", "cu_count", "num_xcc", "fill_us", "check_us", "check2_us",
             "hbm_write_gbps", "hbm_read_gbps", "hbm_bad_words", "hbm_bad_words_pass2", "hbm_first_bad", "mfma_iters",
             "mfma_grid", "mfma_records_ok", "mfma_checksum_mismatch", "mfma_xccs", "mfma_us", "mfma_tflops",
             "clock_mhz_min", "clock_mhz_median", "clock_mhz_max", "total_us", "in_flight_s"],
    "datapath": ["hsa_error", "grid", "cu_count", "num_xcc", "records_ok", "mfma_bad", "tile_bad",
                 "first_bad_got", "first_bad_want", "first_bad_xor", "cus_covered", "simds_covered", "xccs_covered",
                 "kernel_us", "total_us", "in_flight_s"],
}


def _one_shot_check(runtime, kind, devices, nonce, ordinals):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    env = dict(os.environ, ROCR_VISIBLE_DEVICES=str(sorted(ordinals.values())[0]))
    p = subprocess.run([str(probe_executable(runtime)), *_CHECK_FLAGS[kind], "--devices", devices, "--nonce",
                        str(nonce), "--timeout", "20"], stdout=subprocess.PIPE, env=env, timeout=120)
    return p.returncode, json.loads(p.stdout.decode().strip().splitlines()[-1])


@pytest.mark.parametrize("kind", ["sweep", "perf", "datapath"])
def test_check_replies_for_a_missing_gpu_and_a_missing_backend(kind, ordinals):
    """The replies of the whole-chip checks that never reach a device: an
    ordinal past the visible GPUs next to one that runs (HSA build), and the
    HIP build, which has none of these checks."""
    rc, doc = _one_shot_check("hsa", kind, "0,99", 7000, ordinals)
    assert rc == 1 and doc["ok"] is False and doc[kind] is True and doc["hip_device_count"] == 1, doc
    good, missing = doc["devices"]
    assert good["ok"] is True and good["ordinal"] == 0 and good["nonce"] == 7000, good
    assert missing["ok"] is False and missing["ordinal"] == 99 and missing["kept_queue"] is False, missing
    assert missing["error"] == "no such GPU (count=1)", missing
    assert [k for k in _CHECK_COUNTERS[kind] if missing[k] != 0] == [], missing
    if kind == "sweep":
        assert set(missing["wgs_per_xcc"]) == {0} and missing["all_resident"] is False, missing
    elif kind == "perf":
        assert set(missing["xcd_clock_mhz"]) == {0}, missing
    else:
        assert missing["stage_bad"] == [0, 0, 0, 0], missing
        assert missing["first_bad_wg"] == missing["first_bad_stage"] == missing["first_bad_word"] == -1, missing

    rc, doc = _one_shot_check("hip", kind, "0", 7100, ordinals)
    d = doc["devices"][0]
    assert rc == 1 and doc["ok"] is False and d["ok"] is False and d["ordinal"] == 0 and d["nonce"] == 7100, doc
    assert d["error"].endswith("needs the HSA-direct build (mi355x-liveness-probe)"), d
    assert d["error"].startswith(f"--{kind} "), d
    if kind == "sweep":
        assert d["iters"] == 1, d
    elif kind == "perf":
        assert d["bytes"] == 64 << 20 and d["mfma_iters"] == 1024, d
    else:
        assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1, d


def test_monitor_perf_check_on_idle_gpu(inv, ordinals):
    """The health monitor's cadence: liveness, then the throughput check on the
    idle GPU in the same sweep; a healthy MI355X clears every floor."""
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig, HealthMonitor
    from rocm_k8s_device_plugin_amd.topology import Inventory
    accessible = tuple(d for d in inv.devices if d.id in ordinals)
    sub = Inventory(sysfs_root="/sys", devices=accessible, topology=inv.topology, driver_loaded=True,
                    kfd_present=True)
    mon = HealthMonitor(sub, HealthConfig(exporter_socket=None, liveness=True, perf_check_every=1, perf_mib=1024,
                                          perf_mfma_iters=16384, perf_action="unhealthy"),
                        ordinal_map={d.id: ordinals[d.id] for d in accessible})
    # this pytest process holds HIP queues on the GPU from earlier tests, so the
    # kfd process list (rightly) shows it busy; idle detection is CPU-tested
    mon._idle_devices = lambda dev_ids: set(dev_ids)

    async def go():
        await mon.check_once()
        await mon.close()

    asyncio.run(go())
    assert mon.perf_checks == 1
    assert all(state == "ok" for state, _ in mon.perf_verdicts().values()), mon.perf_verdicts()
    assert all(v.health == "Healthy" for v in mon.snapshot().values()), mon.snapshot()
    assert all(d["mfma_tflops"] > 700 for d in mon.perf_last.values()), mon.perf_last


def test_node_labeller_on_real_mi355x():
    """All label kinds on the real node: schema keys present and MI355X values."""
    from rocm_k8s_device_plugin_amd import constants as C
    from rocm_k8s_device_plugin_amd.labeller import labels as L
    lab = L.generate_labels({k: True for k in C.SUPPORTED_LABELS}, "container")
    flat = dict(lab)
    keys = {k.split("/", 1)[1] for k in flat}
    for k in ("gpu.family", "gpu.device-id", "gpu.cu-count", "gpu.vram", "gpu.simd-count",
              "gpu.compute-partitioning-supported", "gpu.memory-partitioning-supported", "gpu.mode"):
        assert any(x.startswith(k) for x in keys), (k, sorted(keys))
    vals = {k.split("/", 1)[1]: v for k, v in flat.items() if k.startswith("amd.com/")}
    assert vals.get("gpu.family") == "AI", vals
    assert vals.get("gpu.device-id") == "75a3" and vals.get("gpu.cu-count") == "256", vals
    assert vals.get("gpu.mode") == "container"
    # additions: gfx950 target, one hive, no xGMI link down on a healthy node
    extra = L.generate_labels({"gfx-target": True, "xgmi-hive-count": True, "xgmi-links-down": True}, "container")
    assert extra.get("amd.com/gpu.gfx-target") == "gfx950", extra
    assert extra.get("amd.com/gpu.xgmi-links-down") == "0", extra
    # driver version: the card's module/version, /sys/module/amdgpu/version or amd-smi
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/labels_gpu_test.json", "w") as f:
        json.dump({"labels": lab, "extra": extra}, f, indent=1)
    assert vals.get("gpu.driver-version"), vals
    assert "(" not in vals["gpu.driver-version"] and len(vals["gpu.driver-version"]) <= 63, vals


def test_smi_cross_check(inv):
    from rocm_k8s_device_plugin_amd.ops.native import core
    n = core()
    if not n.smi_available():
        pytest.skip("libamd_smi not loadable")
    snap = n.smi_snapshot()
    if not snap["ok"]:
        pytest.skip(snap["error"])
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/amdsmi_snapshot.json", "w") as f:
        json.dump(snap, f, indent=1, default=str)
    bdfs = {g["bdf"] for g in snap["gpus"]}
    assert bdfs & {d.bdf for d in inv.devices}
    # GFX activity corroborates pending probes on busy GPUs (health/monitor.py)
    mine = [g for g in snap["gpus"] if g["bdf"] in {d.bdf for d in inv.devices if d.identity == "kfd"}]
    assert mine and all(0 <= g["gfx_activity"] <= 100 for g in mine), mine


def test_drm_gpu_info(inv, ordinals):
    from rocm_k8s_device_plugin_amd.ops.native import core
    n = core()
    if not n.drm_available():
        pytest.skip("libdrm_amdgpu not loadable")
    d = inv.by_id[next(iter(ordinals))]
    # containers usually get only the render node; libdrm works on either
    node = f"card{d.card}" if os.path.exists(f"/dev/dri/card{d.card}") else f"renderD{d.render_minor}"
    info = n.drm_query_gpu_info("/dev", "/sys", node)
    assert info["ok"], info
    assert info["family"] == "AI", info  # gfx9 family (AMDGPU_FAMILY_AI = 141)
    assert info["asic_id"] == d.pci_device_id
    fw = n.drm_query_firmware("/dev", "/sys", node)
    assert fw["ok"] and "MEC" in fw["firmware"]
    with open("gpurun_out/drm_info.json", "w") as f:
        json.dump({"info": info, "fw": fw}, f, indent=1)


def test_end_to_end_admission_container_ready(inv, ordinals):
    """fake kubelet -> plugin (real sysfs) -> Allocate -> container process -> MFMA ready."""
    from rocm_k8s_device_plugin_amd.container_runtime import render_minors_from_specs, start_container
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig
    from rocm_k8s_device_plugin_amd.plugin.container import ContainerImpl
    from rocm_k8s_device_plugin_amd.plugin.manager import ManagerConfig, PluginManager
    from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet
    from rocm_k8s_device_plugin_amd.topology import Inventory

    acc = Inventory(sysfs_root="/sys", devices=tuple(inv.by_id[i] for i in ordinals), topology=inv.topology,
                    driver_loaded=True, kfd_present=True)

    async def go(tmp):
        k = FakeKubelet(tmp)
        await k.start()
        # the health DaemonSet's sources: liveness + amd-smi ECC, events and xGMI link state
        impl = ContainerImpl("single", "/sys", HealthConfig(exporter_socket=None, liveness=True, smi_ecc=True,
                                                            smi_events=True, smi_xgmi=True), inventory=acc)
        mgr = PluginManager(impl, ManagerConfig(pulse_s=0.5, plugin_dir=tmp, handle_signals=False))
        t = asyncio.create_task(mgr.run())
        try:
            await k.wait_for_resource("amd.com/gpu", len(acc), timeout=30)
            adm = await k.admit("amd.com/gpu", 1)
            car = adm.response.container_responses[0]
            minors = render_minors_from_specs(car)
            m2o = {acc.by_id[i].render_minor: o for i, o in ordinals.items()}
            # the container's /dev holds exactly the DeviceSpecs: ROCr sees the pod's GPU only
            r = start_container([m2o[m] for m in minors], device_paths=[ds.host_path for ds in car.devices])
            assert r.ok, r.error
            assert r.t_ready_ns > r.t_start_ns
            assert r.doc["hip_device_count"] == 1
            assert r.doc["devices"][0]["pci_bus_id"].lower() == adm.device_ids[0].lower()
            # the health loop (with liveness) must keep every device Healthy
            st = k.resources["amd.com/gpu"]
            assert all(h == "Healthy" for h in st.devices.values())
            mon = impl.monitor
            assert mon.sweeps >= 1 and mon.fabric is not None and not mon.fabric.error, mon.fabric.error
            assert mon.degraded_links() == frozenset()
        finally:
            mgr.request_stop()
            await t
            await k.stop()

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        asyncio.run(asyncio.wait_for(go(tmp), 120))


@pytest.mark.parametrize("runtime", ["hsa", "hip"])
def test_rocprof_exactly_one_dispatch_per_probe(tmp_path, runtime):
    """SURVEY §2.5 H1 verification: rocprofv3 sees exactly one kernel dispatch per device per probe."""
    import csv
    import shutil
    if not shutil.which("rocprofv3"):
        pytest.skip("rocprofv3 not available")
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    out = tmp_path / "prof"
    env = dict(os.environ, TMPDIR="/tmp")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "probe",
                        "--", str(probe_executable(runtime)), "--devices", "all"], capture_output=True,
                       timeout=300, env=env, cwd="/tmp")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    traces = list(out.rglob("*kernel_trace.csv"))
    assert traces, list(out.rglob("*"))
    rows = list(csv.DictReader(open(traces[0])))
    names = [r["Kernel_Name"] for r in rows]
    doc = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert names == ["mi355x_mfma_liveness"] * len(doc["devices"]), names
    r = rows[0]
    assert (r["Workgroup_Size_X"], r["Grid_Size_X"]) == ("64", "64")
    assert int(r["LDS_Block_Size"]) == 0 and int(r["Scratch_Size"]) == 0


def test_rocprof_kept_queue_server_one_dispatch_per_sweep(tmp_path):
    """--serve --keep under rocprofv3: K sweeps are exactly K liveness dispatches, no runtime blit/fill kernels."""
    import csv
    import shutil
    if not shutil.which("rocprofv3"):
        pytest.skip("rocprofv3 not available")
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    out = tmp_path / "prof"
    sweeps = 16
    reqs = "".join(f"probe 4 5.0 0:{1000 + i}\n" for i in range(sweeps)) + "quit\n"
    env = dict(os.environ, TMPDIR="/tmp")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "serve",
                        "--", str(probe_executable("hsa")), "--serve", "--keep"], input=reqs.encode(),
                       capture_output=True, timeout=300, env=env, cwd="/tmp")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [json.loads(l) for l in p.stdout.decode().splitlines() if l.startswith("{")]
    replies = [d for d in lines if "devices" in d]
    assert len(replies) == sweeps and all(d["ok"] for d in replies)
    assert [d["devices"][0]["setup_us"] > 0 for d in replies] == [True] + [False] * (sweeps - 1)
    traces = list(out.rglob("*kernel_trace.csv"))
    assert traces, list(out.rglob("*"))
    names = [r["Kernel_Name"] for r in csv.DictReader(open(traces[0]))]
    assert names == ["mi355x_mfma_liveness"] * sweeps, names
    os.makedirs("gpurun_out", exist_ok=True)
    shutil.copy(traces[0], "gpurun_out/rocprof_kept_server_kernel_trace.csv")


def test_probe_server_answers_a_burst_of_tagged_requests():
    """The kept-queue server's worker pool (probe_main.cpp serve_worker): 48 tagged probes written at once, with an
    untagged chip sweep among them, each answered once with its own id and nonce; the pool stays bounded; `quit`
    drains it and the server exits 0."""
    import select
    import time
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    p = subprocess.Popen([str(probe_executable("hsa")), "--serve", "--keep"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, cwd="/tmp")
    buf = b""

    def lines_until(pred, timeout):
        nonlocal buf
        got, end = [], time.monotonic() + timeout
        while not pred(got):
            left = end - time.monotonic()
            assert left > 0, f"timed out with {len(got)} replies"
            if "\n" not in buf.decode(errors="replace"):
                r, _, _ = select.select([p.stdout], [], [], left)
                if not r:
                    continue
                chunk = os.read(p.stdout.fileno(), 1 << 16)
                assert chunk, "probe server closed its stdout"
                buf += chunk
                continue
            line, buf = buf.split(b"\n", 1)
            if line.startswith(b"{"):
                got.append(json.loads(line))
        return got

    try:
        hello = lines_until(lambda g: len(g) >= 1, 120)[0]
        assert hello["serve"] and hello["ok"] and hello["concurrent"], hello
        p.stdin.write(b"probe 4 5.0 0:1\n")  # sets the kept queue up
        p.stdin.flush()
        first = lines_until(lambda g: len(g) >= 1, 60)[0]
        assert first["ok"], first
        n = 48
        reqs = [f"@{i} probe 4 5.0 0:{2000 + i}:5.0\n" for i in range(1, n + 1)]
        reqs.insert(n // 2, "sweep 4 5.0 0:77\n")
        p.stdin.write("".join(reqs).encode())
        p.stdin.flush()
        got = lines_until(lambda g: len(g) >= n + 1, 120)
        with open(f"/proc/{p.pid}/status") as f:
            threads = int(next(l for l in f if l.startswith("Threads:")).split()[1])
        tagged = {d["id"]: d for d in got if "id" in d}
        assert sorted(tagged) == list(range(1, n + 1)), sorted(tagged)
        for i, d in tagged.items():
            assert d["ok"] and d["devices"][0]["nonce"] == 2000 + i, d
        sweep = [d for d in got if "id" not in d]
        assert len(sweep) == 1 and sweep[0]["sweep"] and sweep[0]["ok"], sweep
        assert threads <= 64 + 16, threads  # kMaxServeWorkers plus the runtime's own threads
        p.stdin.write(b"quit\n")
        p.stdin.flush()
        assert p.wait(timeout=60) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait(timeout=30)


def test_real_box_matches_mi355x_model(inv):
    """The registry's MI355X numbers against the real part; consistent partitions."""
    from rocm_k8s_device_plugin_amd.models import MI355X, check_inventory, model_for
    readable = [d for d in inv.devices if d.identity == "kfd"]
    for d in readable:
        assert model_for(d.pci_device_id, d.gfx_target_version) is MI355X, hex(d.pci_device_id)
        assert d.cu_count == MI355X.cus_per_partition(d.compute_partition)
        assert abs(d.vram_bytes * MI355X.partitions_per_gpu(d.compute_partition) - MI355X.vram_bytes) \
            < 0.01 * MI355X.vram_bytes
    assert check_inventory(readable) == []


def test_real_fabric_links(inv):
    """Record the kfd io_links of the readable GPU nodes (xGMI type/bandwidth as the driver reports them)."""
    from rocm_k8s_device_plugin_amd.parallel import Fabric
    fab = Fabric(inv)
    links = []
    for nid in inv.topology.gpu_node_ids():
        n = inv.topology.node(nid)
        links += [dict(l, src=nid) for l in n.io_links] + [dict(l, src=nid) for l in n.p2p_links]
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/real_fabric_links.json", "w") as f:
        json.dump({"links": links, "report": fab.report([d.id for d in inv.devices]).as_dict()}, f, indent=1)
    readable = [d for d in inv.devices if d.identity == "kfd"]
    assert readable
    rep = fab.report([readable[0].id])
    assert rep.physical_gpus == 1


def test_collectives_cli_on_rccl():
    """The pod-side collective check on RCCL (one rank: the box has one GPU; the 8-rank run is the driver's)."""
    import socket
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "rocm_k8s_device_plugin_amd.parallel.collectives",
           "--sizes", "1M,64M", "--iters", "5", "--warmup", "2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert {r["op"] for r in rows} == {"all_reduce", "all_gather", "reduce_scatter", "all_to_all"}
    for r in rows:
        assert r["ok"] is True and r["ranks"] == 1 and r["dtype"] == "bfloat16"


_BENCH_RCCL = r"""
import json, torch, torch.distributed as dist
from rocm_k8s_device_plugin_amd.benchmark.coord import Dist
from rocm_k8s_device_plugin_amd.parallel import collectives as coll
d = Dist()
if d.world == 1:            # bench.py creates the gloo world only at N > 1; do it here for one rank
    dist.init_process_group("gloo")
    d.torch, d.dist = torch, dist
group, on_gpu = d.rccl_group()  # what bench.py's collectives stage calls after the timed loop
rows = coll.run([1 << 20, 16 << 20], coll.DEFAULT_OPS, iters=3, warmup=1, dtype=torch.bfloat16, group=group)
print(json.dumps({"backend": dist.get_backend(group), "on_gpu": on_gpu, "cuda": d.cuda, "summary": coll.summary(rows)}))
dist.destroy_process_group()
"""


def test_bench_rccl_group_on_top_of_the_gloo_world(tmp_path):
    """bench.py's collectives stage: an RCCL group created on the GPU after the
    timed loop, on top of the gloo world the ranks coordinate over (one rank
    here; the driver's 8-GPU run uses 8)."""
    import socket
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "bench_rccl.py"
    script.write_text(_BENCH_RCCL)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["backend"] == "nccl" and out["on_gpu"] is True and out["cuda"] is True, out
    summ = out["summary"]
    assert summ["ok"] is True and set(summ["busbw_gbs"]) == {"all_reduce", "all_gather", "reduce_scatter",
                                                             "all_to_all"}, summ


def test_topology_watch_signature_on_real_sysfs():
    """The reload fingerprint reads on the real box (kfd generation_id + partition modes) and is stable."""
    from rocm_k8s_device_plugin_amd.health.monitor import HealthConfig
    from rocm_k8s_device_plugin_amd.plugin.container import ContainerImpl
    impl = ContainerImpl("single", "/sys", HealthConfig(exporter_socket=None))
    gen, parts = impl._signature()
    assert gen is not None and gen.isdigit(), gen
    assert parts and all(cp for _, cp, _ in parts), parts
    assert asyncio.run(impl.reload_topology()) is None
    asyncio.run(impl.close())


def test_xgmi_link_state_on_real_mi355x(inv):
    """amd-smi's live xGMI link state for this GPU: link slots with 7 up on an
    8-GPU MI355X node, peers named by BDF; the watcher's first reading is the
    baseline and degrades nothing."""
    from rocm_k8s_device_plugin_amd.health.fabric import LINK_UP, FabricWatcher
    from rocm_k8s_device_plugin_amd.ops.native import core
    snap = core().smi_xgmi_links()
    assert snap["ok"], snap
    mine = {d.bdf.lower() for d in inv.devices}
    gpus = [g for g in snap["gpus"] if g["bdf"].lower() in mine]
    assert gpus, snap
    for g in gpus:
        assert g["status_ok"], g
        assert sum(s == LINK_UP for s in g["status"]) >= 1, g
        if g["metrics_ok"]:
            assert any(p["peer_bdf"].lower() in mine and p["link_type"] == 2 for p in g["peers"]), g
    w = FabricWatcher(inv)
    w.check()
    assert not w.check() and w.degraded == frozenset()
