"""native/tests/kernel_contract_cli.cpp for the tests: where the built program
is (or a fresh compile of it), and its sweep-verdict / perf-verdict commands
as functions of numpy arrays. Likewise native/tests/probe_contract_cli.cpp
(the probe's reply printers and request grammar).

A case is what the host was handed after a dispatch; a variant is a list of
(array, index, value) word replacements applied to the case for one more
verdict, so "one wrong thing at a time" costs a few bytes, not a copy of a
256-workgroup sweep. Every function returns the parsed JSON lines, the line
for the case as given first.
"""
from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
SOURCE = REPO / "native" / "tests" / "kernel_contract_cli.cpp"
PROBE_SOURCE = REPO / "native" / "tests" / "probe_contract_cli.cpp"
INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

RECORDS, TILES, COUNTERS = 0, 1, 1       # a patch's array: sweep (records, tiles), perf (records, counters)


def host_compiler():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def compile_cli(exe: Path, extra_flags=(), source: Path = SOURCE) -> Path:
    cxx = host_compiler()
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", *extra_flags]
    for inc in INCLUDES:
        cmd += ["-I", str(inc)]
    subprocess.run(cmd + [str(source), "-o", str(exe)], check=True, timeout=300)
    return exe


def contract_cli(build_dir: Path) -> Path:
    """The program the native build left in the package's bin directory when it
    was built from the sources as they are now (the build's content digest, not
    mtimes: a copied tree keeps its binaries), else one compiled into
    `build_dir`. A machine without a compiler runs what was built."""
    from .. import _build
    exe = _build.CONTRACT_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "kernel_contract_cli")


def probe_contract_cli(build_dir: Path) -> Path:
    """native/tests/probe_contract_cli.cpp, found or compiled like contract_cli()."""
    from .. import _build
    exe = _build.PROBE_CONTRACT_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "probe_contract_cli", source=PROBE_SOURCE)


def probe_replies_text(cli, command: str = "replies") -> str:
    """The document `probe_contract_cli replies` (or `replies-bf16`, `replies-fp8`, `replies-f16`) prints, as
    its bytes."""
    r = subprocess.run([str(cli), command], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout


def probe_parse(cli, lines) -> list:
    """`probe_contract_cli parse` over request lines (each with its own line
    end or none): per line the parsed request, or "bad request"."""
    text = "".join(ln if ln.endswith("\n") else ln + "\n" for ln in lines)
    r = subprocess.run([str(cli), "parse"], input=text.encode(), capture_output=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    out = [json.loads(ln) for ln in r.stdout.decode().splitlines()]
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def _variants_blob(variants) -> bytes:
    out = []
    for patches in variants:
        flat = np.asarray([tuple(int(x) & 0xFFFFFFFF for x in p) for p in patches], dtype=np.uint32).reshape(-1, 3)
        out.append(struct.pack("<I", len(flat)) + flat.tobytes())
    return b"".join(out)


def sweep_case(records, tiles, grid: int, nonce: int, iters: int, num_xcc: int, variants=()) -> bytes:
    records = np.ascontiguousarray(records, dtype=np.uint32)
    tiles = np.ascontiguousarray(tiles, dtype=np.float32)
    assert records.size == grid * 16 and tiles.size == grid * 1024, (records.size, tiles.size, grid)
    return (struct.pack("<IIiiI", grid, nonce, iters, num_xcc, len(variants)) + records.tobytes() + tiles.tobytes()
            + _variants_blob(variants))


def perf_case(records, counters, burn_wgs: int, nonce: int, num_xcc: int, bytes: int, mfma_iters: int,  # noqa: A002
              fill_us: float, check_us: float, check2_us: float, mfma_us: float, variants=()) -> bytes:
    records = np.ascontiguousarray(records, dtype=np.uint32)
    counters = np.ascontiguousarray(counters, dtype=np.uint32)
    assert records.size == burn_wgs * 16 and counters.size == 4, (records.size, counters.size, burn_wgs)
    return (struct.pack("<IIiiQddddII", burn_wgs, nonce, num_xcc, mfma_iters, bytes, fill_us, check_us, check2_us,
                        mfma_us, len(variants), 0) + counters.tobytes() + records.tobytes()
            + _variants_blob(variants))


def run_lines(cli, command: str, blob: bytes, expect: int, timeout: float = 300) -> list:
    """The raw output lines of `cli command` fed `blob`; `expect` of them."""
    r = subprocess.run([str(cli), command], input=blob, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    lines = r.stdout.decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == expect, (len(lines) - 1, expect)
    return lines[:-1]


def sweep_verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_lines(cli, "sweep-verdict", b"".join(blobs), expect)]


def perf_verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_lines(cli, "perf-verdict", b"".join(blobs), expect)]
