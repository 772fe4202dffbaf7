#!/usr/bin/env python3
"""Fault-injection stand-in for ``mi355x-liveness-probe`` (CPU tests).

Speaks the same CLI and JSON contract, one-shot and ``--serve``: every reply
has the keys, the order and the JSON types of the real probe's printers, and a
request line is accepted or refused ("bad request", and the server goes on) as
the real parser does (tests/test_probe_contract.py holds both to
native/tests/probe_contract_cli.cpp). Behaviour
per ROCr ordinal comes from the JSON file named by $MI355X_STUB_PROBE_CONTROL
(re-read on every request), e.g.
``{"0": "ok", "3": "fail", "5": "hang", "6": "stale", "7": "garbage"}``
(missing ordinals are "ok"; "serve": "broken" makes --serve fail to start,
"serve": "slow_start" delays its hello by "serve_start_s" seconds;
"server_fail" fails only inside --serve: a stale server runtime; "slow" is a
dispatch that completes "slow_s" seconds after it was submitted: in --serve a
request whose deadline comes first is answered pending and a later one collects
the late verdict; "pending" keeps the dispatch queued and, like the real server,
answers only when the device's deadline has passed).
--serve speaks the real server's protocol: "@<id>"-tagged requests answered
concurrently with their id, per-device deadlines ("<ordinal>:<nonce>:<s>"),
requests on one device serialised on its slot.
Exercises the real LivenessProber code path: process spawn, server protocol,
deadline kill, fallback to per-device isolation, output parsing, nonce check,
hysteresis. Each start appends a line to $MI355X_STUB_PROBE_LOG if set.
Chip-sweep replies ("sweep" requests / --sweep) are sweep-shaped and follow the
control file's "sweep" map, e.g. ``{"sweep": {"3": "mfma_bad", "4": "missing_xcd"}}``,
and the ordinal's plain mode (see _sweep_device and serve()).
Throughput-check replies ("perf" requests / --perf) follow the control file's
"perf" map, e.g. ``{"perf": {"3": "slow_xcd", "4": "corrupt"}}``.
MFMA datapath-check replies ("datapath" requests / --datapath) follow the
"datapath" map, e.g. ``{"datapath": {"2": "stuck_bit", "5": "missing"}}``; each
one appends "datapath:<host ordinal>" to $MI355X_STUB_PROBE_LOG.
int8 MFMA datapath-check replies ("datapath_i8" requests / --datapath-i8)
follow the "datapath_i8" map with the same modes; each one appends
"datapath_i8:<host ordinal>" to $MI355X_STUB_PROBE_LOG.
bf16 MFMA datapath-check replies ("datapath_bf16" requests / --datapath-bf16)
follow the "datapath_bf16" map, likewise, and append "datapath_bf16:<host ordinal>".
fp8 / MX-scaled MFMA datapath-check replies ("datapath_fp8" requests /
--datapath-fp8) follow the "datapath_fp8" map and append "datapath_fp8:<host ordinal>".
f16 MFMA datapath-check replies ("datapath_f16" requests /
--datapath-f16) follow the "datapath_f16" map and append "datapath_f16:<host ordinal>".
Each iteration count it is asked for (a "probe" / "sweep" request line, or
--iters) is appended to $MI355X_STUB_PROBE_ITERS_LOG if set, as "<kind> <iters>".
Every line --serve reads and every line it writes back is appended to
$MI355X_STUB_PROBE_REQUEST_LOG if set, as "> <request line>" and "< <reply>":
what reached the server and what it said, whether or not the caller still
waited for it. The log changes no reply.
Two control keys are for the prober's late-verdict bookkeeping alone:
"reply_delay_s" holds every --serve reply back that long (a reply its caller has
stopped waiting for), and "late_nonce" ({ordinal: nonce}) makes the device's next
verdicts late ones that carry that nonce (a dispatch this server never got).
"""
import json
import os
import re
import sys
import time


def _control():
    path = os.environ.get("MI355X_STUB_PROBE_CONTROL")
    if path and os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def _identity(ordinal, kind="probe"):
    """Agent identity per host ordinal from $MI355X_STUB_PROBE_IDENTITY (JSON
    {ordinal: {"kfd_node_id": N, "pci_bus_id": "dddd:bb:dd.f"}}); unknown otherwise,
    and for the kinds $MI355X_STUB_PROBE_ANONYMOUS lists ("probe,sweep,.."): a
    probe that names no agent in those replies."""
    raw = os.environ.get("MI355X_STUB_PROBE_IDENTITY")
    ident = json.loads(raw).get(str(ordinal), {}) if raw else {}
    if kind in os.environ.get("MI355X_STUB_PROBE_ANONYMOUS", "").split(","):
        ident = {}
    return {"kfd_node_id": int(ident.get("kfd_node_id", -1)), "pci_bus_id": ident.get("pci_bus_id", "")}


# Every reply below has the keys of the real probe's printer (native/src/health/probe_json.h),
# in its order and with its JSON types; tests/test_probe_contract.py compares them with
# `probe_contract_cli replies`. The figures of the fault modes are the shipped verdict's on the
# records testing/probe_contract.py builds for each mode (for its NONCE; the request's is echoed).
def _device(ordinal_reported, mode, nonce, host_ordinal=None, iters=4):
    ok = mode == "ok"
    who = _identity(ordinal_reported if host_ordinal is None else host_ordinal)
    return {"ordinal": ordinal_reported, "ok": ok or mode == "stale", "hip_error": 0, "mismatches": 0 if ok else 17,
            "nonce": nonce if mode != "stale" else (nonce + 1) & 0xFFFFFFFF, "xcc_id": 0, "hw_id": 0, "iters": iters,
            "dispatches": 1, "kfd_node_id": who["kfd_node_id"], "runtime": "stub", "kernel_us": 3.0, "setup_us": 1.0,
            "total_us": 5.0, "phase_us": {"code_object": 0.5, "queue": 0.25, "buffers": 0.0, "dispatch_wait": 3.5},
            "pci_bus_id": who["pci_bus_id"], "arch": "gfx950", "name": "", "uuid": "", "pci_domain": 0,
            "pci_bus": 0, "pci_device": 0, "cu_count": 256, "total_mem": 0, "late": False, "pending_s": 0.0,
            "error": "" if ok or mode == "stale" else "17/1024 MFMA results differ from host reference"}


DATAPATH_KINDS = ("datapath", "datapath_i8", "datapath_bf16", "datapath_fp8", "datapath_f16")


def _log_check(kind, host_ordinal):
    log = os.environ.get("MI355X_STUB_PROBE_LOG")
    if log and kind in DATAPATH_KINDS:
        with open(log, "a") as f:
            f.write(f"{kind}:{host_ordinal}\n")


SWEEP_FAULTS = {
    "mfma_bad": dict(records_ok=255, mfma_bad=12, all_resident=False,
                     error="255/256 workgroups correct (mfma_bad=12 lds_bad=0 tile_bad=0), 8/8 XCDs ran"),
    "lds_bad": dict(records_ok=255, lds_bad=3, all_resident=False,
                    error="255/256 workgroups correct (mfma_bad=0 lds_bad=3 tile_bad=0), 8/8 XCDs ran"),
    "tile_bad": dict(records_ok=255, tile_bad=1, all_resident=False,
                     error="255/256 workgroups correct (mfma_bad=0 lds_bad=0 tile_bad=1), 8/8 XCDs ran"),
    "missing": dict(records_ok=255, cus_covered=255, all_resident=False, wgs_per_xcc=[32, 31, 32, 32, 32, 32, 32, 32],
                    error="255/256 workgroups correct (mfma_bad=0 lds_bad=0 tile_bad=0), 8/8 XCDs ran"),
    "missing_xcd": dict(xccs_covered=7, wgs_per_xcc=[37, 37, 37, 37, 36, 36, 36, 0],
                        error="256/256 workgroups correct (mfma_bad=0 lds_bad=0 tile_bad=0), 7/8 XCDs ran"),
}


def _sweep_device(ordinal_reported, mode, nonce, host_ordinal=None, iters=4):
    """Chip-sweep reply (kind "sweep"); modes from the control file's "sweep"
    map: mfma_bad / lds_bad (one CU's device-side compare), tile_bad (one wrong
    word in one CU's tile), missing (one workgroup wrote no record), missing_xcd
    (one XCD ran nothing). An ordinal's plain mode counts too: fail (as
    tile_bad), stale (a wrong nonce); see serve() for hang, pending, slow."""
    who = _identity(ordinal_reported if host_ordinal is None else host_ordinal, "sweep")
    d = {"ordinal": ordinal_reported, "ok": mode in ("ok", "stale"), "hsa_error": 0,
         "nonce": nonce if mode != "stale" else (nonce + 1) & 0xFFFFFFFF, "iters": iters, "grid": 256, "cu_count": 256,
         "num_xcc": 8, "records_ok": 256, "mfma_bad": 0, "lds_bad": 0, "tile_bad": 0, "cus_covered": 256,
         "xccs_covered": 8, "all_resident": True, "wgs_per_xcc": [32] * 8, "kernel_us": 300.0,
         "arrival_spread_us": 2.55, "total_us": 1500.0, "in_flight_s": 0.0, "kept_queue": True, **who, "error": ""}
    if mode in SWEEP_FAULTS:
        d.update(SWEEP_FAULTS[mode])
    elif mode == "fail":
        d.update(SWEEP_FAULTS["tile_bad"])
    return d


def _perf_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """Throughput-check reply (kind "perf"); modes from the control file's
    "perf" map: slow_hbm, slow_mfma, slow_xcd (one XCD at a third of the clock),
    slow_xcd_after_absent (five XCDs, XCD 0 reports no clock, XCD 3 is slow),
    corrupt (HBM words read back wrong); hang (the server never answers; serve mode only)."""
    who = _identity(ordinal_reported if host_ordinal is None else host_ordinal, "perf")
    xcd = [1530.0] * 8
    if mode == "slow_xcd":
        xcd[3] = 510.0
    if mode == "slow_xcd_after_absent":
        xcd = [0.0, 2400.0, 2400.0, 900.0, 2400.0]
    read, tflops = (1500.0 if mode == "slow_hbm" else 6000.0), (400.0 if mode == "slow_mfma" else 1550.0)
    bad = 3 if mode == "corrupt" else 0
    clocks = sorted(c for c in xcd if c > 0)
    return {"ordinal": ordinal_reported, "ok": mode != "corrupt", "hsa_error": 0, "nonce": nonce, "bytes": 4 << 30,
            "cu_count": 256, "num_xcc": len(xcd), "fill_us": 933.7, "check_us": (4 << 30) / (read * 1e3),
            "check2_us": (4 << 30) / (read * 1e3), "hbm_write_gbps": 4600.0, "hbm_read_gbps": read,
            "hbm_bad_words": bad, "hbm_bad_words_pass2": bad, "hbm_first_bad": 4096 if bad else -1,
            "mfma_iters": 65536, "mfma_grid": 512, "mfma_records_ok": 512, "mfma_checksum_mismatch": 0,
            "mfma_xccs": len(xcd), "mfma_us": 8796093.022208 / tflops, "mfma_tflops": tflops, "clock_mhz_min": clocks[0],
            "clock_mhz_median": clocks[len(clocks) // 2], "clock_mhz_max": clocks[-1], "xcd_clock_mhz": xcd,
            "total_us": 35000.0, "in_flight_s": 0.0, "kept_queue": True, **who,
            "error": "hbm_bad_words=3 first_bad_unit=4096 mfma records 512/512 checksum mismatches 0, 8/8 XCDs ran"
                     if bad else ""}


def _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, stages, stuck, kernel_us, total_us, kind=None):
    who = _identity(ordinal_reported if host_ordinal is None else host_ordinal,
                    kind or ("datapath" if stages == 4 else "datapath_i8"))
    d = {"ordinal": ordinal_reported, "ok": mode == "ok", "hsa_error": 0, "nonce": nonce, "grid": 256, "cu_count": 256,
         "num_xcc": 8, "records_ok": 256, "mfma_bad": 0, "stage_bad": [0] * stages, "tile_bad": 0,
         "first_bad_wg": -1, "first_bad_stage": -1, "first_bad_word": -1, "first_bad_got": 0, "first_bad_want": 0,
         "first_bad_xor": 0, "cus_covered": 256, "simds_covered": 1024, "xccs_covered": 8, "kernel_us": kernel_us,
         "total_us": total_us, "in_flight_s": 0.0, "kept_queue": True, **who, "error": ""}
    if mode == "stuck_bit":
        d.update(stuck)
    elif mode == "missing":
        d.update(records_ok=254, cus_covered=254, simds_covered=1016,
                 error="254/256 workgroups exact (device_bad=0 tile_bad=0)")
    elif mode == "device_bad":
        bad = [0] * stages
        bad[1 if stages == 4 else 4] = 12
        d.update(records_ok=255, mfma_bad=12, stage_bad=bad, error="255/256 workgroups exact (device_bad=12 tile_bad=0)")
    return d


def _datapath_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """MFMA datapath-check reply (kind "datapath"); modes from the control
    file's "datapath" map: stuck_bit (bit 30 of every stage-2 word of one CU's
    tile stuck at 0: the first wrong word is named), missing (two workgroups wrote
    no record), device_bad (the device-side compare found mismatches); hang (the
    server never answers; serve mode only)."""
    stuck = dict(records_ok=255, tile_bad=774, first_bad_wg=17, first_bad_stage=2, first_bad_word=5,
                 first_bad_got=0x80A67530, first_bad_want=0xC0A67530, first_bad_xor=0x40000000,
                 error="255/256 workgroups exact (device_bad=0 tile_bad=774); first bad: wg 17 stage 2 word 5 "
                       "xor 0x40000000 (bit 30)")
    return _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, 4, stuck, 20.0, 900.0)


def _datapath_i8_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """int8 MFMA datapath-check reply (kind "datapath_i8"); the modes of
    _datapath_device, from the control file's "datapath_i8" map (stuck_bit: bit
    30 of every stage-4 word of one CU's tile)."""
    stuck = dict(records_ok=255, tile_bad=129, first_bad_wg=17, first_bad_stage=4, first_bad_word=5,
                 first_bad_got=0x8CE47D32, first_bad_want=0xCCE47D32, first_bad_xor=0x40000000,
                 error="255/256 workgroups exact (device_bad=0 tile_bad=129); first bad: wg 17 stage 4 word 5 "
                       "xor 0x40000000 (bit 30)")
    return _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, 5, stuck, 25.0, 2000.0)


def _datapath_bf16_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """bf16 MFMA datapath-check reply (kind "datapath_bf16"); the modes of
    _datapath_device, from the control file's "datapath_bf16" map (stuck_bit: bit
    30 of every stage-4 word of one CU's tile)."""
    stuck = dict(records_ok=255, tile_bad=196, first_bad_wg=17, first_bad_stage=4, first_bad_word=0,
                 first_bad_got=0x02A8F830, first_bad_want=0x42A8F830, first_bad_xor=0x40000000,
                 error="255/256 workgroups exact (device_bad=0 tile_bad=196); first bad: wg 17 stage 4 word 0 "
                       "xor 0x40000000 (bit 30)")
    return _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, 5, stuck, 30.0, 2500.0, kind="datapath_bf16")


def _datapath_fp8_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """fp8 / MX-scaled MFMA datapath-check reply (kind "datapath_fp8"; eight
    stages); the modes of _datapath_device, from the control file's
    "datapath_fp8" map (stuck_bit: bit 30 of every stage-4 word of one CU's tile)."""
    stuck = dict(records_ok=255, tile_bad=473, first_bad_wg=17, first_bad_stage=4, first_bad_word=0,
                 first_bad_got=0x98800000, first_bad_want=0xD8800000, first_bad_xor=0x40000000,
                 error="255/256 workgroups exact (device_bad=0 tile_bad=473); first bad: wg 17 stage 4 word 0 "
                       "xor 0x40000000 (bit 30)")
    return _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, 8, stuck, 60.0, 3000.0, kind="datapath_fp8")


def _datapath_f16_device(ordinal_reported, mode, nonce, host_ordinal=None):
    """f16 MFMA datapath-check reply (kind "datapath_f16"; seven stages); the
    modes of _datapath_device, from the control file's "datapath_f16" map
    (stuck_bit: bit 30 of every stage-4 word of one CU's tile)."""
    stuck = dict(records_ok=255, tile_bad=207, first_bad_wg=17, first_bad_stage=4, first_bad_word=0,
                 first_bad_got=0x0DE9F070, first_bad_want=0x4DE9F070, first_bad_xor=0x40000000,
                 error="255/256 workgroups exact (device_bad=0 tile_bad=207); first bad: wg 17 stage 4 word 0 "
                       "xor 0x40000000 (bit 30)")
    return _datapath_reply(ordinal_reported, mode, nonce, host_ordinal, 7, stuck, 35.0, 2600.0, kind="datapath_f16")


CHECK_DEVICE = {"sweep": _sweep_device, "perf": _perf_device, "datapath": _datapath_device,
                "datapath_i8": _datapath_i8_device, "datapath_bf16": _datapath_bf16_device,
                "datapath_fp8": _datapath_fp8_device,
                "datapath_f16": _datapath_f16_device}


def _blank(kind, ordinal_reported, nonce=0):
    """A check's reply before anything is known (probe_json.h blank_result)."""
    d = CHECK_DEVICE[kind](ordinal_reported, "ok", nonce)
    for k, v in d.items():
        if k not in ("ordinal", "nonce"):
            d[k] = False if isinstance(v, bool) else 0 if isinstance(v, int) else 0.0 if isinstance(v, float) else \
                "" if isinstance(v, str) else [0] * (len(v) if k == "stage_bad" else 8)
    d.update({k: -1 for k in ("first_bad_wg", "first_bad_stage", "first_bad_word") if k in d}, kfd_node_id=-1)
    return d


def _not_completed(kind, ordinal_reported, nonce, host_ordinal, in_flight_s, error, iters=4):
    """A check (not a probe) whose dispatch has not completed: nothing counted,
    hsa_error -1; in_flight_s > 0 when an earlier one is still outstanding
    (hsa_chip.cpp Check::begin / Check::run)."""
    d = _blank(kind, ordinal_reported, nonce)
    d.update(_identity(ordinal_reported if host_ordinal is None else host_ordinal, kind), hsa_error=-1,
             in_flight_s=in_flight_s, error=error)
    if kind == "sweep":
        d["iters"] = iters
    return d


def _kfd_entry():
    """Like a kept-queue server: a kfd proc entry with one queue per GPU id
    (MI355X_STUB_KFD_PROC / MI355X_STUB_KFD_GPUIDS), removed on exit.
    MI355X_STUB_KFD_ALSO="<pid>:<gid>,<gid>" adds another process' entry in the
    same instant (a pod started with the server; left in place)."""
    root, gids = os.environ.get("MI355X_STUB_KFD_PROC"), os.environ.get("MI355X_STUB_KFD_GPUIDS", "")
    if not root:
        return None
    import shutil

    def make(entry, ids):
        for i, g in enumerate(x for x in ids.split(",") if x):
            os.makedirs(os.path.join(entry, "queues", str(i)), exist_ok=True)
            with open(os.path.join(entry, "queues", str(i), "gpuid"), "w") as f:
                f.write(g + "\n")
    entry = os.path.join(root, str(os.getpid()))
    make(entry, gids)
    also = os.environ.get("MI355X_STUB_KFD_ALSO", "")
    if also:
        pid, ids = also.split(":")
        make(os.path.join(root, pid), ids)
    import atexit
    atexit.register(shutil.rmtree, entry, True)
    return entry


def _log_wire(mark, text):
    path = os.environ.get("MI355X_STUB_PROBE_REQUEST_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{mark} {text}\n")


def _log_iters(kind, iters):
    path = os.environ.get("MI355X_STUB_PROBE_ITERS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{kind} {iters}\n")


_INT = r"\s*([+-]?\d+)"
_UINT0 = r"\s*([+-]?(?:0[xX][0-9a-fA-F]+|0[0-7]*|[1-9]\d*))"   # strtoul, base 0
_FLOAT = r"\s*([+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)"   # strtod / %lf, decimal forms
# like sscanf, field by field: each takes all it can and gives nothing back to the next
_HEADS = (("perf", (_INT, _FLOAT, _UINT0)), ("datapath_i8", (_FLOAT,)), ("datapath_bf16", (_FLOAT,)),
          ("datapath_fp8", (_FLOAT,)),
          ("datapath_f16", (_FLOAT,)),
          ("datapath", (_FLOAT,)),
          ("sweep", (_INT, _FLOAT)), ("probe", (_INT, _FLOAT)))
_DEVICE = re.compile(_INT + ":" + _UINT0 + "(?::" + _FLOAT + ")?")


def _c_uint(text):
    """strtoul(text, base 0) as a uint32_t."""
    neg, digits = text.startswith("-"), text.lstrip("+-")
    v = int(digits, 8) if len(digits) > 1 and digits[1] not in "xX" and digits[0] == "0" else int(digits, 0)
    return (-v if neg else v) & 0xFFFFFFFF


def _parse_tagged(line):
    """(request or None, tagged, id) of one request line without its line end,
    by the grammar of native/src/health/probe_request.h: a line that parser
    refuses is None here. tests/test_probe_contract.py runs one corpus through both."""
    tagged, rid = False, 0
    if line.startswith("@"):
        m = re.match(r"@\s*(\+?\d+) ", line)
        if not m:
            return None, False, 0
        tagged, rid, line = True, int(m.group(1)), line[m.end():]
    for kind, head in _HEADS:
        if line.startswith(kind + " "):
            break
    else:
        return None, tagged, rid
    rest, g = line[len(kind):], []
    for field in head:
        m = re.match(field, rest)
        if not m:
            return None, tagged, rid
        g.append(m.group(1))
        rest = rest[m.end():]
    req = {"tagged": tagged, "id": rid, "kind": kind, "iters": int(g[0]) if len(g) > 1 else 0,
           "timeout": float(g[-1] if len(g) < 3 else g[1]), "mib": _c_uint(g[2]) if len(g) > 2 else 0, "devices": []}
    rest = rest.lstrip()
    while rest:
        d = _DEVICE.match(rest)
        if not d:            # text left over after the device list: no part of the request is answered
            return None, tagged, rid
        dl = float(d.group(3)) if d.group(3) is not None else 0.0
        req["devices"].append([int(d.group(1)), _c_uint(d.group(2)), dl if dl > 0 else req["timeout"]])
        rest = rest[d.end():].lstrip(" ")
    return req, tagged, rid


def _parse(line):
    """One request line: {"tagged", "id", "kind", "iters", "timeout", "mib",
    "devices": [[ordinal, nonce, deadline_s], ..]} as `probe_contract_cli parse`
    prints it, or "bad request"."""
    req, _, _ = _parse_tagged(line.rstrip("\r\n"))
    return "bad request" if req is None else req


def _envelope(kind, ok, count, devices, rid=None):
    """The line around a --serve reply's devices (probe_json.h serve_reply_json)."""
    doc = {"ok": ok, "hip_device_count": count, "sweep": kind == "sweep", "perf": kind == "perf",
           "t_ready_ns": time.monotonic_ns()}
    if kind in DATAPATH_KINDS:
        doc[kind] = True
    doc["devices"] = devices
    return doc if rid is None else {"id": rid, **doc}


def _bad_request(tagged, rid):
    return {**({"id": rid} if tagged else {}), "ok": False, "error": "bad request", "devices": []}


def serve():
    import threading
    ctl = _control()
    t = time.monotonic_ns()
    if ctl.get("serve") == "broken":
        print(json.dumps({"serve": True, "ok": False, "hip_device_count": 0, "concurrent": True, "deadlines": True,
                          "t_start_ns": t, "t_runtime_ns": t}), flush=True)
        return 2
    if ctl.get("serve") == "slow_start":   # a runtime start-up that outlasts the caller's patience
        time.sleep(float(ctl.get("serve_start_s", 30)))
    _kfd_entry()
    t = time.monotonic_ns()
    # like the real server: tagged requests are answered concurrently, as they complete
    print(json.dumps({"serve": True, "ok": True, "hip_device_count": 8, "concurrent": True, "deadlines": True,
                      "t_start_ns": t, "t_runtime_ns": t}), flush=True)
    slots = {}   # ordinal -> (nonce, iters) of the kept slot's outstanding dispatch (like --keep)
    slow = {}    # ordinal -> (submitted at, nonce, iters) of a "slow" device's outstanding dispatch
    flying = {}  # ordinal -> when a sweep that did not complete was submitted (at most one per device)
    locks = {}   # ordinal -> its kept slot's lock (requests on one device serialise, as on the real server)
    out_mu, state_mu = threading.Lock(), threading.Lock()
    # like ROCr: with ROCR_VISIBLE_DEVICES the server numbers only those GPUs
    vis = [x for x in os.environ.get("ROCR_VISIBLE_DEVICES", "").split(",") if x]
    starts_log = os.environ.get("MI355X_STUB_PROBE_LOG")
    if starts_log and vis:
        with open(starts_log, "a") as f:
            f.write("visible=" + ",".join(vis) + "\n")

    def host_of(o):
        return vis[o] if vis and 0 <= o < len(vis) else str(o)

    def one(req, o, n, deadline, ctl):
        kind, iters = req["kind"], req["iters"]
        hosto = host_of(o)
        if not 0 <= o < 8:   # run_batch / run_on_each: a blank result with the reason
            if kind == "probe":
                d = _device(o, "fail", 0, iters=0)
                d.update(mismatches=0, runtime="", arch="", cu_count=0, kernel_us=0.0, setup_us=0.0, total_us=0.0,
                         dispatches=0, kfd_node_id=0, pci_bus_id="", error="no such GPU (count=8)",
                         phase_us=dict.fromkeys(d["phase_us"], 0.0))
                return d
            d = _blank(kind, o)
            d["error"] = "no such GPU (count=8)"
            return d
        if kind == "perf" or kind in DATAPATH_KINDS:
            mode = ctl.get(kind, {}).get(hosto, "ok")
            if mode == "hang":   # a check that never finishes (the daemon stops meanwhile)
                time.sleep(3600)
            return CHECK_DEVICE[kind](o, mode, n, host_ordinal=int(hosto))
        mode = ctl.get(hosto, "ok")
        if mode == "server_fail":
            mode = "fail"
        if mode == "hang":
            time.sleep(3600)
        if mode == "garbage":
            print("segfault-ish noise", flush=True)
            os._exit(139)
        if kind == "sweep":
            # the sweep's own dispatch (a probe left "pending" on the kept slot
            # does not hold it up): one that does not complete within the
            # device's deadline ("timeout"; "slow" while "slow_s" is longer) is
            # abandoned, and until it completes no other is submitted: the
            # reply says for how long it has been in flight
            with state_mu:
                since = flying.get(o)
                if since is not None and (mode not in ("timeout", "slow") or
                                          (mode == "slow" and time.monotonic() - since >= float(ctl.get("slow_s", 1.0)))):
                    del flying[o]   # it completed meanwhile
                    since = None
            if since is not None:
                s = max(time.monotonic() - since, 1e-3)
                return _not_completed("sweep", o, n, int(hosto), s, iters=iters,
                                      error=f"earlier chip sweep / check still in flight for {s:.1f}s (not completed)")
            if mode == "timeout" or (mode == "slow" and float(ctl.get("slow_s", 1.0)) > deadline):
                with state_mu:
                    flying[o] = time.monotonic()
                time.sleep(deadline)
                return _not_completed("sweep", o, n, int(hosto), 0.0, iters=iters,
                                      error=f"chip sweep did not complete within {deadline:.1f}s")
            if mode == "slow":
                time.sleep(float(ctl.get("slow_s", 1.0)))
            if mode in ("slow", "pending"):
                mode = "ok"
            smode = ctl.get("sweep", {}).get(hosto, "ok")
            return _sweep_device(o, smode if mode == "ok" else mode, n, host_ordinal=int(hosto), iters=iters)
        if mode == "slow":
            # a dispatch that completes "slow_s" seconds after it was submitted:
            # a request whose deadline comes first is answered pending (the
            # dispatch stays queued), and a later one collects its late verdict
            with state_mu:
                since, first, first_iters = slow.setdefault(o, (time.monotonic(), n, iters))
            left = since + float(ctl.get("slow_s", 1.0)) - time.monotonic()
            if left > deadline:
                time.sleep(deadline)
                d = _device(o, "fail", n, host_ordinal=int(hosto), iters=iters)
                d.update(hip_error=-1, mismatches=0, pending_s=max(time.monotonic() - since, 1e-3),
                         error=f"dispatch pending for {time.monotonic() - since:.1f}s (not completed)")
                return d
            time.sleep(max(0.0, left))
            with state_mu:
                slow.pop(o, None)
            # the verdict names the dispatch it is about: its nonce and its iteration count
            d = _device(o, "ok", first, host_ordinal=int(hosto), iters=first_iters)
            d["late"] = first != n
            return d
        if mode == "timeout":   # server without kept queues: the dispatch did not complete
            time.sleep(deadline)
            d = _device(o, "fail", n, host_ordinal=int(hosto), iters=iters)
            d.update(hip_error=-1, mismatches=0, error=f"dispatch did not complete within {deadline:.1f}s")
            return d
        if mode == "pending":
            # kept-queue server: the dispatch stays queued behind other work; the
            # server waits out this device's whole deadline first, as
            # hsa_probe.cpp's wait_and_verify does
            with state_mu:
                slots.setdefault(o, (n, iters))
            if starts_log:   # a test can tell when a request is waiting on this device
                with open(starts_log, "a") as f:
                    f.write(f"pending:{hosto}\n")
            time.sleep(deadline)
            d = _device(o, "fail", n, host_ordinal=int(hosto), iters=iters)
            d.update(hip_error=-1, mismatches=0, pending_s=max(deadline, 1e-3),
                     error=f"dispatch pending for {deadline:.1f}s (not completed)")
            return d
        with state_mu:
            late = slots.pop(o, None)
        if late is None and hosto in ctl.get("late_nonce", {}):
            late = (int(ctl["late_nonce"][hosto]), iters)
        if late is not None:   # the outstanding dispatch completed: its late verdict
            d = _device(o, mode, late[0], host_ordinal=int(hosto), iters=late[1])
            d["late"] = True
            return d
        return _device(o, mode, n, host_ordinal=int(hosto), iters=iters)

    def answer(req):
        ctl = _control()
        kind, devs_in = req["kind"], req["devices"]
        res = [None] * len(devs_in)

        def dev(i, o, n, dl):
            with state_mu:
                lk = locks.setdefault(o, threading.Lock())
            if not lk.acquire(timeout=dl):   # another request holds this device's slot past our deadline
                why = "another request on this device's queue"
                if kind == "probe":
                    d = _device(o, "fail", n, host_ordinal=int(host_of(o)), iters=req["iters"])
                    d.update(hip_error=-1, mismatches=0, pending_s=dl, error=why)
                else:
                    d = _not_completed(kind, o, n, int(host_of(o)), dl, why)
                res[i] = d
                return
            try:
                res[i] = one(req, o, n, dl, ctl)
            finally:
                lk.release()
        for o, _, _ in devs_in:   # in request order, before the devices run side by side
            _log_check(kind, host_of(o))
        ths = [threading.Thread(target=dev, args=(i, *x), daemon=True) for i, x in enumerate(devs_in)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        # like the real server: a request that names no device is not ok
        doc = _envelope(kind, bool(res) and all(d["ok"] for d in res), 8, res, req["id"] if req["tagged"] else None)
        time.sleep(float(ctl.get("reply_delay_s", 0)))
        with out_mu:
            _log_wire("<", json.dumps(doc))
            sys.stdout.write(json.dumps(doc) + "\n")
            sys.stdout.flush()

    workers = []
    for line in sys.stdin:
        line = line.rstrip("\r\n")
        if not line:
            continue
        _log_wire(">", line)
        if line == "quit":
            break
        req, tagged, rid = _parse_tagged(line)
        if req is None:      # the real server says so and goes on
            with out_mu:
                _log_wire("<", json.dumps(_bad_request(tagged, rid)))
                sys.stdout.write(json.dumps(_bad_request(tagged, rid)) + "\n")
                sys.stdout.flush()
            continue
        if req["kind"] in ("probe", "sweep"):
            _log_iters(req["kind"], req["iters"])
        if not tagged:
            answer(req)
        else:
            workers.append(threading.Thread(target=answer, args=(req,), daemon=True))
            workers[-1].start()
    # like the real server, answer what was accepted before leaving (it waits for its
    # workers up to a minute; a test's stuck device must not hold the stub that long)
    leave_by = time.monotonic() + 2.0
    for th in workers:
        th.join(max(0.0, leave_by - time.monotonic()))
    return 0


def main(argv):
    log = os.environ.get("MI355X_STUB_PROBE_LOG")
    if log:
        with open(log, "a") as f:
            f.write(("serve" + ("+keep" if "--keep" in argv else "") if "--serve" in argv
                     else os.environ.get("ROCR_VISIBLE_DEVICES", "0")) + "\n")
    if "--serve" in argv:
        return serve()
    iters = 4
    if "--iters" in argv:
        iters = int(argv[argv.index("--iters") + 1])
        _log_iters("sweep" if "--sweep" in argv else "probe", iters)
    nonce = 0
    for i, a in enumerate(argv):
        if a == "--nonce":
            nonce = int(argv[i + 1], 0)
    ordinal = os.environ.get("ROCR_VISIBLE_DEVICES", "0").split(",")[0]
    t = time.monotonic_ns()
    ctl = _control()
    mode = ctl.get(ordinal, "ok")
    for flag, kind in (("--perf", "perf"), ("--datapath", "datapath"), ("--datapath-i8", "datapath_i8"),
                       ("--datapath-bf16", "datapath_bf16"), ("--datapath-fp8", "datapath_fp8"),
                       ("--datapath-f16", "datapath_f16"),
                       ("--sweep", "sweep")):
        if flag not in argv:
            continue
        if kind == "sweep":
            if mode == "hang":
                time.sleep(3600)
            smode = ctl.get("sweep", {}).get(ordinal, "ok") if mode in ("ok", "server_fail", "slow") else \
                "fail" if mode in ("pending", "timeout") else mode
            d = _sweep_device(0, smode, nonce, host_ordinal=int(ordinal), iters=iters)
        else:
            _log_check(kind, ordinal)
            d = CHECK_DEVICE[kind](0, ctl.get(kind, {}).get(ordinal, "ok"), nonce, host_ordinal=int(ordinal))
        # probe_json.h oneshot_check_json
        print(json.dumps({"ok": d["ok"], kind: True, "hip_device_count": 1, "t_start_ns": t, "t_runtime_ns": t,
                          "t_ready_ns": time.monotonic_ns(), "devices": [d]}))
        return 0 if d["ok"] else 1
    if mode == "server_fail":
        mode = "ok"
    if mode == "slow":
        time.sleep(float(ctl.get("slow_s", 1.0)))
        mode = "ok"
    if mode in ("pending", "timeout"):   # a fresh process waits too, then gives up
        mode = "fail"
    if mode == "hang":
        time.sleep(3600)
    if mode == "garbage":
        print("segfault-ish noise")
        return 139
    # as a container entrypoint (bench.py --fixture): one result per --devices
    # entry; with the fake runtime's /dev view the visible GPU count is the
    # number of render nodes it allows (what ROCr's thunk would find)
    wanted = ["0"]
    if "--devices" in argv:
        wanted = [x for x in argv[argv.index("--devices") + 1].split(",") if x]
    allow = os.environ.get("MI355X_DEV_ALLOW")
    count = (sum(1 for p in allow.split(";") if "/renderD" in p) if allow is not None
             else max(1, len(wanted)))
    host = os.environ.get("ROCR_VISIBLE_DEVICES")
    devs = [_device(int(o), mode, nonce + i, host_ordinal=int(host.split(",")[int(o)])
                    if host and int(o) < len(host.split(",")) else None, iters=iters)
            for i, o in enumerate(wanted)]
    ok = all(d["ok"] for d in devs)
    # probe_json.h oneshot_probe_json
    doc = {"ok": ok, "hip_device_count": count, "identify": False, "t_start_ns": t, "t_runtime_ns": t,
           "t_ready_ns": time.monotonic_ns(), "cpu_ms_runtime": 0.0, "cpu_user_ms_runtime": 0.0, "cpu_ms_ready": 0.0,
           "read_syscalls_runtime": 0,
           "init_us": {"dlopen": 0.0, "kfd_open": 0.0, "hsa_init": 0.0, "agents": 0.0, "pools": 0.0},
           "init_profile": None, "view": None, "devices": devs}
    print(json.dumps(doc))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
