"""Raw launcher for the kernels of liveness_gfx950.hsaco: every byte a kernel
wrote, saved as .npy, with guard regions around every buffer.

    python -m rocm_k8s_device_plugin_amd.testing.raw_kernels REQUESTS.json OUTDIR

REQUESTS.json is a list of requests, run in order:

    {"id": ..., "kernel": "liveness", "nonce": n, "iters": k}
    {"id": ..., "kernel": "sweep", "nonce": n, "iters": k, "grid": g, "wait_ticks": t[, "args_grid": a]}
        (g workgroups are launched and sized for; the kernel is told a, default g: with a > g the
        residency wait can only end at wait_ticks)
    {"id": ..., "kernel": "hbm_fill", "n16": u, "grid": g, "threads": t, "seed": s, "poison_unit": p | null}
    {"id": ..., "kernel": "hbm_check", "n16": u, "grid": g, "threads": t, "seed": s, "buf_npy": file}
    {"id": ..., "kernel": "burn", "nonce": n, "iters": k, "grid": g, "hbm_counters": [4 words]}
    {"id": ..., "kernel": "datapath", "nonce": n, "grid": g}
    {"id": ..., "kernel": "datapath_i8", "nonce": n, "grid": g}
    {"id": ..., "kernel": "datapath_bf16", "nonce": n, "grid": g[, "launch_grid": workgroups launched, >= g]}
    {"id": ..., "kernel": "datapath_fp8", "nonce": n, "grid": g[, "launch_grid": workgroups launched, >= g]}
    {"id": ..., "kernel": "datapath_f16", "nonce": n, "grid": g[, "launch_grid": workgroups launched, >= g]}

A sweep, datapath, datapath_i8, datapath_bf16, datapath_fp8 or datapath_f16 request may add "code_object": "inject": the kernel then comes from
liveness_gfx950_inject.hsaco, the test-only build of the same sources whose argument structs end in
the injection fields (MI355X_TEST_INJECT in liveness_kernel.h / datapath_kernel.h / datapath_i8_kernel.h /
datapath_bf16_kernel.h / datapath_fp8_kernel.h / datapath_f16_kernel.h), and may add

    "inject": {"kind": "mfma" | "lds", "wg": w, "wave": v, "lane": l, "index": i, "mask": m}

(one data word xor-ed with m: accumulator register i of that lane after the last MFMA -- for the
datapath kernels i = stage * 16 + register -- or LDS pattern word i; wave and lane are unused for "lds").
Without "inject" the hook is off. Every other request uses the production code object.

For each request OUTDIR gets <id>.<buffer>.npy and <id>.<buffer>.canary.npy
(2 x CANARY_BYTES: the guard before and after the buffer), and OUTDIR/status.json
names the completed requests, each one's launch-to-synchronize time ("launch_us", measured, never
judged here) and the first error. The launcher stops at the
first HIP error, or at any non-success from the synchronize after a kernel,
writes what it has, and exits non-zero; it never retries.

A ctypes wrapper over one libamdhip64: the ROCm installation's, which the
project's own binaries link. torch brings a second HIP/ROCr pair, so this
module must run in a process that has not imported torch. Kernel arguments are
packed by ctypes.Structure mirrors of the structs in liveness_kernel.h (the
kernels use explicit arguments only), and passed as one kernarg buffer.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

CANARY_BYTES = 4096
CANARY_FILL = 0xA5
OUT_PREFILL = 0xFF

_u32, _i32, _u64, _ptr = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64


class LivenessArgs(ctypes.Structure):
    _fields_ = [("out", _ptr), ("meta", _ptr), ("scratch", _ptr), ("nonce", _u32), ("iters", _i32)]


class SweepArgs(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("arrive", _ptr), ("nonce", _u32), ("iters", _i32),
                ("grid", _u32), ("wait_ticks", _u32)]


class HbmArgs(ctypes.Structure):
    _fields_ = [("buf", _ptr), ("n16", _u64), ("bad", _ptr), ("first_bad", _ptr), ("threads", _u64),
                ("poison_unit", _u64), ("seed", _u32), ("pad", _u32)]


class BurnArgs(ctypes.Structure):
    _fields_ = [("records", _ptr), ("hbm_counters", _ptr), ("hbm_counters_host", _ptr), ("nonce", _u32),
                ("iters", _i32)]


ARG_STRUCTS = {"mi355x_liveness_args": LivenessArgs, "mi355x_sweep_args": SweepArgs,
               "mi355x_hbm_args": HbmArgs, "mi355x_burn_args": BurnArgs}

class DatapathArgs(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("nonce", _u32), ("grid", _u32)]


# the mirrors of datapath_kernel.h (native/tests/datapath_contract_cli.cpp prints that header's layout)
DATAPATH_ARG_STRUCTS = {"mi355x_datapath_args": DatapathArgs}

_INJECT_FIELDS = [("inject_kind", _u32), ("inject_wg", _u32), ("inject_wave", _u32), ("inject_lane", _u32),
                  ("inject_index", _u32), ("inject_mask", _u32)]


class SweepInjectArgs(ctypes.Structure):
    _fields_ = SweepArgs._fields_ + _INJECT_FIELDS


class DatapathInjectArgs(ctypes.Structure):
    _fields_ = DatapathArgs._fields_ + _INJECT_FIELDS


# the same structs as the test-only code object sees them (`inject-layout` of the two contract programs
# compiled with -DMI355X_TEST_INJECT=1)
INJECT_ARG_STRUCTS = {"mi355x_sweep_args": SweepInjectArgs}
DATAPATH_INJECT_ARG_STRUCTS = {"mi355x_datapath_args": DatapathInjectArgs}


class DatapathI8Args(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("nonce", _u32), ("grid", _u32)]


class DatapathI8InjectArgs(ctypes.Structure):
    _fields_ = DatapathI8Args._fields_ + _INJECT_FIELDS


# the mirrors of datapath_i8_kernel.h (native/tests/datapath_i8_contract_cli.cpp prints that header's layouts)
DATAPATH_I8_ARG_STRUCTS = {"mi355x_datapath_i8_args": DatapathI8Args}
DATAPATH_I8_INJECT_ARG_STRUCTS = {"mi355x_datapath_i8_args": DatapathI8InjectArgs}
DATAPATH_I8_WG_WORDS = 4 * 32 * 32 + 16 * 16         # wave 0's five tiles of one workgroup


class DatapathBf16Args(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("nonce", _u32), ("grid", _u32)]


class DatapathBf16InjectArgs(ctypes.Structure):
    _fields_ = DatapathBf16Args._fields_ + _INJECT_FIELDS


# the mirrors of datapath_bf16_kernel.h (native/tests/datapath_bf16_contract_cli.cpp prints that header's layouts)
DATAPATH_BF16_ARG_STRUCTS = {"mi355x_datapath_bf16_args": DatapathBf16Args}
DATAPATH_BF16_INJECT_ARG_STRUCTS = {"mi355x_datapath_bf16_args": DatapathBf16InjectArgs}
DATAPATH_BF16_WG_WORDS = 4 * 32 * 32 + 16 * 16       # wave 0's five tiles of one workgroup


class DatapathFp8Args(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("nonce", _u32), ("grid", _u32)]


class DatapathFp8InjectArgs(ctypes.Structure):
    _fields_ = DatapathFp8Args._fields_ + _INJECT_FIELDS


# the mirrors of datapath_fp8_kernel.h (native/tests/datapath_fp8_contract_cli.cpp prints that header's layouts)
DATAPATH_FP8_ARG_STRUCTS = {"mi355x_datapath_fp8_args": DatapathFp8Args}
DATAPATH_FP8_INJECT_ARG_STRUCTS = {"mi355x_datapath_fp8_args": DatapathFp8InjectArgs}
DATAPATH_FP8_WG_WORDS = 6 * 32 * 32 + 2 * 16 * 16    # wave 0's eight tiles of one workgroup


class DatapathF16Args(ctypes.Structure):
    _fields_ = [("records", _ptr), ("tiles", _ptr), ("nonce", _u32), ("grid", _u32)]


class DatapathF16InjectArgs(ctypes.Structure):
    _fields_ = DatapathF16Args._fields_ + _INJECT_FIELDS


# the mirrors of datapath_f16_kernel.h (native/tests/datapath_f16_contract_cli.cpp prints that header's layouts)
DATAPATH_F16_ARG_STRUCTS = {"mi355x_datapath_f16_args": DatapathF16Args}
DATAPATH_F16_INJECT_ARG_STRUCTS = {"mi355x_datapath_f16_args": DatapathF16InjectArgs}
DATAPATH_F16_WG_WORDS = 5 * 32 * 32 + 2 * 16 * 16    # wave 0's seven tiles of one workgroup
INJECT_KINDS = {"none": 0, "mfma": 1, "lds": 2}      # MI355X_INJECT_*; the datapath kernel knows none and mfma
CODE_OBJECTS = ("production", "inject")


def inject_words(req: dict) -> tuple:
    """The six trailing argument words of a request for the inject build."""
    inj = req.get("inject")
    if inj is None:
        return (INJECT_KINDS["none"], 0, 0, 0, 0, 0)
    kind = INJECT_KINDS[inj["kind"]]
    if req["kernel"] in ("datapath", "datapath_i8", "datapath_bf16", "datapath_fp8",
                         "datapath_f16") and inj["kind"] == "lds":
        raise ValueError("the datapath kernels have no lds injection")
    return (kind, int(inj["wg"]), int(inj.get("wave", 0)), int(inj.get("lane", 0)), int(inj["index"]),
            int(inj["mask"]) & 0xFFFFFFFF)


def code_object_of(req: dict) -> str:
    which = req.get("code_object", "production")
    if which not in CODE_OBJECTS:
        raise ValueError(f"unknown code object {which!r}")
    if which == "inject" and req["kernel"] not in ("sweep", "datapath", "datapath_i8", "datapath_bf16", "datapath_fp8",
                                                   "datapath_f16"):
        raise ValueError(f"the inject build has no hook in {req['kernel']!r}")
    if which != "inject" and "inject" in req:
        raise ValueError("an injection needs \"code_object\": \"inject\"")
    return which


# kernel -> (symbol, lanes per workgroup)
KERNELS = {"liveness": ("mi355x_mfma_liveness", 64), "sweep": ("mi355x_chip_sweep", 256),
           "hbm_fill": ("mi355x_hbm_fill", 256), "hbm_check": ("mi355x_hbm_check", 256),
           "burn": ("mi355x_mfma_burn", 256), "datapath": ("mi355x_mfma_datapath", 256),
           "datapath_i8": ("mi355x_mfma_datapath_i8", 256),
           "datapath_bf16": ("mi355x_mfma_datapath_bf16", 256),
           "datapath_fp8": ("mi355x_mfma_datapath_fp8", 256),
           "datapath_f16": ("mi355x_mfma_datapath_f16", 256)}

_H2D, _D2H = 1, 2
_LAUNCH_PARAM_BUFFER_POINTER, _LAUNCH_PARAM_BUFFER_SIZE, _LAUNCH_PARAM_END = 1, 2, 3


def hip_library_path() -> str:
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")


class HipError(RuntimeError):
    pass


class Hip:
    def __init__(self):
        if "torch" in sys.modules:
            raise RuntimeError("raw_kernels must not share a process with torch (a second HIP runtime)")
        self.lib = ctypes.CDLL(hip_library_path())
        self.lib.hipGetErrorString.restype = ctypes.c_char_p
        self.lib.hipGetErrorString.argtypes = [ctypes.c_int]
        self.lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipFree.argtypes = [ctypes.c_void_p]
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipModuleLoad.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p]
        self.lib.hipModuleGetFunction.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_char_p]
        self.lib.hipModuleLaunchKernel.argtypes = [ctypes.c_void_p] + [ctypes.c_uint] * 7 + [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def check(self, what: str, status: int) -> None:
        if status != 0:
            raise HipError(f"{what}: hipError {status}: {self.lib.hipGetErrorString(status).decode(errors='replace')}")

    def call(self, name: str, *args) -> None:
        self.check(name, getattr(self.lib, name)(*args))


class Buffer:
    """`initial` bytes of device memory between two CANARY_BYTES guard regions."""

    def __init__(self, hip: Hip, name: str, dtype, initial: bytes):
        assert len(initial) % 4 == 0 and len(initial) > 0
        self.hip, self.name, self.dtype, self.nbytes = hip, name, np.dtype(dtype), len(initial)
        guard = bytes([CANARY_FILL]) * CANARY_BYTES
        image = guard + initial + guard
        base = ctypes.c_void_p()
        hip.call("hipMalloc", ctypes.byref(base), len(image))
        self.base = base.value
        self.ptr = self.base + CANARY_BYTES
        hip.call("hipMemcpy", self.base, image, len(image), _H2D)

    def read(self):
        """(content, canaries) as they are on the device now."""
        host = ctypes.create_string_buffer(self.nbytes + 2 * CANARY_BYTES)
        self.hip.call("hipMemcpy", host, self.base, len(host), _D2H)
        raw = np.frombuffer(host.raw, dtype=np.uint8)
        data = raw[CANARY_BYTES:CANARY_BYTES + self.nbytes].copy().view(self.dtype)
        return data, np.stack([raw[:CANARY_BYTES], raw[CANARY_BYTES + self.nbytes:]])

    def free(self):
        self.hip.call("hipFree", self.base)


def _filled(nbytes: int, byte: int) -> bytes:
    return bytes([byte]) * nbytes


def plan(req: dict, base_dir: Path):
    """(buffer specs [(name, dtype, initial bytes)], args builder, workgroups) of a request."""
    k = req["kernel"]
    code_object_of(req)                  # refuses a build or an injection the kernel does not have
    if k == "liveness":
        bufs = [("out", np.float32, _filled(32 * 32 * 4, OUT_PREFILL)), ("meta", np.uint32, _filled(16, 0)),
                ("scratch", np.float32, _filled(16 * 64 * 4, OUT_PREFILL))]
        return bufs, lambda p: LivenessArgs(p["out"], p["meta"], p["scratch"], req["nonce"], req["iters"]), 1
    if k == "sweep":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, 0)), ("tiles", np.float32, _filled(g * 32 * 32 * 4, OUT_PREFILL)),
                ("arrive", np.uint32, _filled(4, 0))]
        args_grid = int(req.get("args_grid", g))
        if code_object_of(req) == "inject":
            return bufs, lambda p: SweepInjectArgs(p["records"], p["tiles"], p["arrive"], req["nonce"], req["iters"],
                                                   args_grid, req["wait_ticks"], *inject_words(req)), g
        return bufs, lambda p: SweepArgs(p["records"], p["tiles"], p["arrive"], req["nonce"], req["iters"],
                                         args_grid, req["wait_ticks"]), g
    if k in ("hbm_fill", "hbm_check"):
        n16 = int(req["n16"])
        if k == "hbm_fill":
            content = _filled(n16 * 16, 0x5A)
            poison = req.get("poison_unit")
            poison = 0xFFFFFFFFFFFFFFFF if poison is None else int(poison)
        else:
            path = Path(req["buf_npy"])
            arr = np.load(path if path.is_absolute() else base_dir / path)
            assert arr.dtype == np.uint32 and arr.size == 4 * n16, (arr.dtype, arr.size, n16)
            content = arr.tobytes()
            poison = 0xFFFFFFFFFFFFFFFF
        bufs = [("buf", np.uint32, content), ("bad", np.uint32, _filled(4, 0)),
                ("first_bad", np.uint64, _filled(8, 0xFF))]
        return bufs, lambda p: HbmArgs(p["buf"], n16, p["bad"], p["first_bad"], int(req["threads"]), poison,
                                       req["seed"], 0), int(req["grid"])
    if k == "burn":
        g = int(req["grid"])
        counters = np.asarray(req["hbm_counters"], dtype=np.uint32)
        assert counters.size == 4
        bufs = [("records", np.uint32, _filled(g * 16 * 4, 0)), ("hbm_counters", np.uint32, counters.tobytes()),
                ("hbm_counters_host", np.uint32, _filled(16, 0))]
        return bufs, lambda p: BurnArgs(p["records"], p["hbm_counters"], p["hbm_counters_host"], req["nonce"],
                                        req["iters"]), g
    if k == "datapath":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, OUT_PREFILL)),
                ("tiles", np.uint32, _filled(g * 4 * 32 * 32 * 4, OUT_PREFILL))]
        if code_object_of(req) == "inject":
            return bufs, lambda p: DatapathInjectArgs(p["records"], p["tiles"], req["nonce"], g, *inject_words(req)), g
        return bufs, lambda p: DatapathArgs(p["records"], p["tiles"], req["nonce"], g), g
    if k == "datapath_i8":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, OUT_PREFILL)),
                ("tiles", np.uint32, _filled(g * DATAPATH_I8_WG_WORDS * 4, OUT_PREFILL))]
        if code_object_of(req) == "inject":
            return bufs, lambda p: DatapathI8InjectArgs(p["records"], p["tiles"], req["nonce"], g,
                                                        *inject_words(req)), g
        return bufs, lambda p: DatapathI8Args(p["records"], p["tiles"], req["nonce"], g), g
    if k == "datapath_bf16":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, OUT_PREFILL)),
                ("tiles", np.uint32, _filled(g * DATAPATH_BF16_WG_WORDS * 4, OUT_PREFILL))]
        if code_object_of(req) == "inject":
            return bufs, lambda p: DatapathBf16InjectArgs(p["records"], p["tiles"], req["nonce"], g,
                                                          *inject_words(req)), g
        # the buffers hold `grid` workgroups; the ones launched beyond it must write nothing
        wgs = int(req.get("launch_grid", g))
        if wgs < g:
            raise ValueError("launch_grid below grid")
        return bufs, lambda p: DatapathBf16Args(p["records"], p["tiles"], req["nonce"], g), wgs
    if k == "datapath_fp8":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, OUT_PREFILL)),
                ("tiles", np.uint32, _filled(g * DATAPATH_FP8_WG_WORDS * 4, OUT_PREFILL))]
        if code_object_of(req) == "inject":
            return bufs, lambda p: DatapathFp8InjectArgs(p["records"], p["tiles"], req["nonce"], g,
                                                         *inject_words(req)), g
        # the buffers hold `grid` workgroups; the ones launched beyond it must write nothing
        wgs = int(req.get("launch_grid", g))
        if wgs < g:
            raise ValueError("launch_grid below grid")
        return bufs, lambda p: DatapathFp8Args(p["records"], p["tiles"], req["nonce"], g), wgs
    if k == "datapath_f16":
        g = int(req["grid"])
        bufs = [("records", np.uint32, _filled(g * 16 * 4, OUT_PREFILL)),
                ("tiles", np.uint32, _filled(g * DATAPATH_F16_WG_WORDS * 4, OUT_PREFILL))]
        if code_object_of(req) == "inject":
            return bufs, lambda p: DatapathF16InjectArgs(p["records"], p["tiles"], req["nonce"], g,
                                                         *inject_words(req)), g
        # the buffers hold `grid` workgroups; the ones launched beyond it must write nothing
        wgs = int(req.get("launch_grid", g))
        if wgs < g:
            raise ValueError("launch_grid below grid")
        return bufs, lambda p: DatapathF16Args(p["records"], p["tiles"], req["nonce"], g), wgs
    raise ValueError(f"unknown kernel {k!r}")


def run_request(hip: Hip, functions: dict, req: dict, base_dir: Path, outdir: Path) -> float:
    """Runs one request; the launch-to-synchronize time in microseconds."""
    specs, make_args, wgs = plan(req, base_dir)
    symbol, lanes = KERNELS[req["kernel"]]
    bufs = [Buffer(hip, name, dtype, initial) for name, dtype, initial in specs]
    args = make_args({b.name: b.ptr for b in bufs})
    size = ctypes.c_size_t(ctypes.sizeof(args))
    extra = (ctypes.c_void_p * 5)(_LAUNCH_PARAM_BUFFER_POINTER, ctypes.addressof(args), _LAUNCH_PARAM_BUFFER_SIZE,
                                  ctypes.addressof(size), _LAUNCH_PARAM_END)
    t0 = time.perf_counter_ns()
    hip.call("hipModuleLaunchKernel", functions[symbol], wgs, 1, 1, lanes, 1, 1, 0, None, None, extra)
    hip.call("hipDeviceSynchronize")
    launch_us = (time.perf_counter_ns() - t0) / 1e3
    for b in bufs:
        data, canary = b.read()
        np.save(outdir / f"{req['id']}.{b.name}.npy", data)
        np.save(outdir / f"{req['id']}.{b.name}.canary.npy", canary)
    for b in bufs:
        b.free()
    return launch_us


def load_functions(hip: Hip, path) -> dict:
    """symbol -> function handle of every kernel of one code object."""
    module = ctypes.c_void_p()
    hip.call("hipModuleLoad", ctypes.byref(module), str(path).encode())
    functions = {}
    for symbol, _ in KERNELS.values():
        f = ctypes.c_void_p()
        hip.call("hipModuleGetFunction", ctypes.byref(f), module, symbol.encode())
        functions[symbol] = f
    return functions


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    req_path, outdir = Path(argv[0]).resolve(), Path(argv[1])
    requests = json.loads(req_path.read_text())
    outdir.mkdir(parents=True, exist_ok=True)
    status = {"completed": [], "launch_us": {}, "error": None, "failed": None, "hip_library": hip_library_path()}
    current = None
    try:
        from rocm_k8s_device_plugin_amd import _build
        hip = Hip()
        hip.call("hipInit", 0)
        hip.call("hipSetDevice", int(os.environ.get("MI355X_RAW_DEVICE", "0")))
        paths = {"production": _build.HSACO, "inject": _build.HSACO_INJECT}
        loaded = {"production": load_functions(hip, paths["production"])}
        for req in requests:
            current = req["id"]
            which = code_object_of(req)
            if which not in loaded:          # the test-only build is loaded only for a request that names it
                loaded[which] = load_functions(hip, paths[which])
            status["launch_us"][current] = run_request(hip, loaded[which], req, req_path.parent, outdir)
            status["completed"].append(current)
        current = None
    except Exception as e:  # noqa: BLE001 - the first error ends the run, whatever it is
        status["error"], status["failed"] = f"{type(e).__name__}: {e}", current
    (outdir / "status.json").write_text(json.dumps(status, indent=1))
    if status["error"]:
        print(f"raw_kernels: stopped at {status['failed'] or 'start-up'}: {status['error']}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
