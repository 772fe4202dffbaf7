"""Independent reference for the MFMA datapath check (mi355x_mfma_datapath,
native/src/health/datapath_kernel.h, datapath_verify.h).

Written from the recipe in the header's comment, in Python ints and
`fractions.Fraction`: operands are built as exact rationals and encoded into
IEEE-754 binary32 words by a codec that refuses anything it cannot represent
exactly as a normal number, so "exact by construction" is checked here, not
assumed. Nothing below uses float arithmetic.

Also: the record / tile image a correct kernel writes, the verdict the host
draws from them, wrong-kernel and stuck-bit models, and a driver for
native/tests/datapath_contract_cli.cpp.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
from fractions import Fraction
from functools import lru_cache
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
CLI_SOURCE = REPO / "native" / "tests" / "datapath_contract_cli.cpp"
CLI_INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

M32 = 0xFFFFFFFF
ROWS = COLS = 32
DEPTH = 2
STAGES = 4
TILE_WORDS = ROWS * COLS
WG_WORDS = STAGES * TILE_WORDS
REC_WORDS = 16
WAVES = 4
THREADS = 256
MAGIC = int.from_bytes(b"DPTH", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8

# the nonces of the issue: small ones, and the ones where nonce arithmetic wraps
NONCES = (0, 1, 6, 7, 12345, 0xDEADBEEF, 0xFFFFFFF9, 0xFFFFFFFF)
WG_WAVES = ((0, 0), (3, 1), (255, 3))

GOLDEN, MURMUR = 0x9E3779B1, 0x85EBCA77
SEL_A, SEL_B, SEL_C, SEL_ROW, SEL_COL = 0x0000, 0x0100, 0x1000, 0x2000, 0x3000
BAND = range(97, 159)          # exponent fields of a full-band word
WIDE = range(1, 255)           # of a stage-3 C word
POWERS = range(-90, 91)        # selector powers of two
SCALES = range(-40, 41)        # stage-2 row / column scales


# ---- binary32 codec over exact rationals ---------------------------------------
def decode(word: int) -> Fraction:
    """The value of a binary32 word that is zero or a normal number."""
    sign, field, frac = word >> 31, word >> 23 & 0xFF, word & 0x7FFFFF
    if field == 0 and frac == 0:
        return Fraction(0)
    assert 1 <= field <= 254, f"{word:#010x} is subnormal, Inf or NaN"
    mag = Fraction(0x800000 | frac) * Fraction(2) ** (field - 150)
    return -mag if sign else mag


def encode(value: Fraction) -> int:
    """The binary32 word of a non-zero value; refuses a value that is not
    exactly a normal binary32 number."""
    assert value != 0, "zero has two encodings: not decided here"
    sign, num, den = int(value < 0), abs(value.numerator), value.denominator
    assert den & (den - 1) == 0, f"{value} is no binary fraction"
    log2 = num.bit_length() - den.bit_length()            # floor(log2(|value|)): den is a power of two
    lift = 23 - log2 - (den.bit_length() - 1)             # |value| = significand * 2^(log2 - 23)
    assert lift >= 0 or num % (1 << -lift) == 0, f"{value} needs more than 24 significant bits"
    significand = num << lift if lift >= 0 else num >> -lift
    field = log2 + 127
    assert 1 <= field <= 254, f"{value} is outside the normal range"
    return sign << 31 | field << 23 | (significand & 0x7FFFFF)


def is_normal(value: Fraction) -> bool:
    try:
        encode(value)
    except AssertionError:
        return False
    return True


# ---- integer hashes ---------------------------------------------------------------
def wave_nonce(nonce: int, wg: int, wave: int) -> int:
    return ((nonce ^ wg * GOLDEN & M32) + wave * MURMUR) & M32


def mix(nw: int, stage: int, selector: int) -> int:
    h = nw ^ ((stage + 1) * GOLDEN & M32) ^ (selector * MURMUR & M32)
    for shift, mult in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h ^= h >> shift
        h = h * mult & M32
    return h ^ h >> 16


def _banded(nw: int, stage: int, selector: int, offset: int, fields: range) -> int:
    """Any sign, any mantissa, exponent field within `fields`; the word at
    offset 1 is the bitwise complement of the word at offset 0."""
    h = mix(nw, stage, selector + (0 if offset == 1 else offset))
    word = h & 0x80000000 | fields[(h >> 23 & 0xFF) % len(fields)] << 23 | h & 0x7FFFFF
    return word ^ M32 if offset == 1 else word


def _power(h: int, powers: range) -> Fraction:
    mag = Fraction(2) ** powers[(h & 0x7FFFFFFF) % len(powers)]
    return -mag if h >> 31 else mag


def _odd(h: int) -> int:
    """A signed integer congruent to 1 modulo 4, magnitude below 2^11."""
    body = h & 0x7FC
    return -(body + 3) if h >> 31 else body + 1


def _scale(nw: int, selector: int, index: int) -> Fraction:
    return Fraction(2) ** SCALES[mix(nw, 2, selector + index) % len(SCALES)]


def a_word(stage: int, i: int, k: int, nw: int) -> int:
    if stage == 0:
        return _banded(nw, 0, SEL_A, 2 * i + k, BAND)
    if stage == 1:
        return encode(_power(mix(nw, 1, SEL_ROW + i), POWERS)) if k == i % 2 else 0
    if stage == 2:
        return encode(_odd(mix(nw, 2, SEL_A + 2 * i + k)) * _scale(nw, SEL_ROW, i))
    return 0


def b_word(stage: int, k: int, j: int, nw: int) -> int:
    if stage == 0:
        return encode(_power(mix(nw, 0, SEL_COL + j), POWERS)) if k == j % 2 else 0
    if stage == 2:
        return encode(_odd(mix(nw, 2, SEL_B + COLS * k + j)) * _scale(nw, SEL_COL, j))
    return _banded(nw, stage, SEL_B, COLS * k + j, BAND)


def c_word(stage: int, i: int, j: int, nw: int) -> int:
    if stage == 2:
        h = mix(nw, 2, SEL_C + COLS * i + j)
        q = 4 * ((h & 0x7FFFFFFF) % 0xFFFFF + 1)
        return encode((-q if h >> 31 else q) * _scale(nw, SEL_ROW, i) * _scale(nw, SEL_COL, j))
    if stage == 3:
        return _banded(nw, 3, SEL_C, COLS * i + j, WIDE)
    return 0


@lru_cache(maxsize=None)
def operands(stage: int, nw: int):
    """(A words [32][2], B words [2][32], C words [32][32]) of one wave's stage."""
    a = tuple(tuple(a_word(stage, i, k, nw) for k in range(DEPTH)) for i in range(ROWS))
    b = tuple(tuple(b_word(stage, k, j, nw) for j in range(COLS)) for k in range(DEPTH))
    c = tuple(tuple(c_word(stage, i, j, nw) for j in range(COLS)) for i in range(ROWS))
    return a, b, c


def exactness_violations(stage: int, nw: int) -> list:
    """Every way one wave's stage breaks the exactness contract: a non-zero
    product or a partial sum (in either k order) that is not a normal binary32
    number, a zero partial sum after a non-zero term, or a zero output."""
    a, b, c = operands(stage, nw)
    av = [[decode(w) for w in row] for row in a]
    bv = [[decode(w) for w in row] for row in b]
    out = []
    for i in range(ROWS):
        for j in range(COLS):
            prods = [av[i][k] * bv[k][j] for k in range(DEPTH)]
            for k, p in enumerate(prods):
                if p != 0 and not is_normal(p):
                    out.append((stage, i, j, f"product k={k}"))
            for order in ((0, 1), (1, 0)):
                acc, moved = decode(c[i][j]), c[i][j] != 0
                for k in order:
                    acc, moved = acc + prods[k], moved or prods[k] != 0
                    if (moved or acc != 0) and not is_normal(acc):
                        out.append((stage, i, j, f"partial sum order={order} after k={k}"))
                if acc == 0:
                    out.append((stage, i, j, "zero output"))
    return out


@lru_cache(maxsize=None)
def expected_tile(stage: int, nw: int) -> tuple:
    """The 1024 output words of one wave's stage, row-major: C + A·B in exact
    rational arithmetic, encoded (so it must be exactly representable)."""
    a, b, c = operands(stage, nw)
    av = [[decode(w) for w in row] for row in a]
    bv = [[decode(w) for w in row] for row in b]
    return tuple(encode(decode(c[i][j]) + sum(av[i][k] * bv[k][j] for k in range(DEPTH)))
                 for i in range(ROWS) for j in range(COLS))


def toggle_masks(nw: int) -> dict:
    """Per operand, the bits that take both values over one wave's tile set."""
    def both(words):
        words = list(words)
        ones = zeros = 0
        for w in words:
            ones, zeros = ones | w, zeros | (w ^ M32)
        return ones & zeros
    a0, _, _ = operands(0, nw)
    _, b1, _ = operands(1, nw)
    _, _, c3 = operands(3, nw)
    return {"A": both(w for row in a0 for w in row), "B": both(w for row in b1 for w in row),
            "C": both(w for row in c3 for w in row),
            "D": both(w for s in range(STAGES) for w in expected_tile(s, nw))}


# ---- what a correct kernel writes ----------------------------------------------------
_tiles_cache: dict = {}


def tiles_image(nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][stage][32][32] as uint32: wave 0's four tiles of every
    workgroup. Computed once per (nonce, grid) and read-only: copy before changing it."""
    key = (nonce, grid)
    if key not in _tiles_cache:
        t = np.array([[expected_tile(s, wave_nonce(nonce, wg, 0)) for s in range(STAGES)] for wg in range(grid)],
                     dtype=np.uint32).reshape(grid, STAGES, ROWS, COLS)
        t.setflags(write=False)
        _tiles_cache[key] = t
    return _tiles_cache[key]


def spread_placement(grid: int, xcds: int = 8) -> list:
    """(xcc, cu-bits) per workgroup: dealt round-robin to the XCDs."""
    return [(wg % xcds, wg // xcds) for wg in range(grid)]


def healthy(grid: int, nonce: int, placement=None):
    """(records, tiles) a correct mi355x_mfma_datapath would write; wave v of a
    workgroup on SIMD v of its CU."""
    placement = list(placement or spread_placement(grid))
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        recs[wg, REC_MAGIC], recs[wg, REC_WG], recs[wg, REC_NONCE], recs[wg, REC_XCC] = MAGIC, wg, nonce ^ wg, xcc
        for v in range(WAVES):
            recs[wg, REC_HWID + v] = cu << 8 | v << 4 | 0x1
    return recs, tiles_image(nonce, grid).copy()


ACC_REGS = 16


def accumulator_element(lane: int, reg: int) -> tuple:
    """(row, column) of a stage's 32x32 tile that accumulator register `reg` of
    lane `lane` holds: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def injection_image(nonce: int, grid: int, inject=None) -> tuple:
    """(stage_bad (grid, 4), tiles (grid, 4, 32, 32) uint32) that
    mi355x_mfma_datapath of the test-only build must leave behind under `inject`
    (a raw_kernels request's "inject" object: index = stage * 16 + register;
    None for the hook off), from the documented layout alone. The wrong word is
    counted once, by its workgroup, in its stage's counter; it reaches the
    host's tiles only from wave 0, and there it differs from the healthy word by
    exactly the mask. An index outside 0..63 injects nothing."""
    stage_bad = np.zeros((grid, STAGES), dtype=np.int64)
    tiles = tiles_image(nonce, grid).copy()
    if inject is not None and inject["mask"] & M32 and inject["wg"] < grid:
        assert inject["kind"] == "mfma", inject
        wg, wave, lane, index = inject["wg"], inject["wave"], inject["lane"], inject["index"]
        if wave < WAVES and lane < 64 and index < STAGES * ACC_REGS:
            stage, reg = divmod(index, ACC_REGS)
            stage_bad[wg, stage] = 1
            if wave == 0:
                i, j = accumulator_element(lane, reg)
                tiles[wg, stage, i, j] ^= np.uint32(inject["mask"] & M32)
    return stage_bad, tiles


HW_WORDS = (REC_XCC, REC_HWID, REC_HWID + 1, REC_HWID + 2, REC_HWID + 3)   # hardware's, not the reference's


def check_raw(records, tiles, nonce: int, grid: int, inject=None) -> None:
    """Every word the kernel wrote against the reference image: the whole tile
    buffer, and the records but for where the workgroup ran (those: XCC id in
    range, HW_ID words non-zero). `inject`: the injection the test-only build
    was asked for (injection_image)."""
    rec = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)
    til = np.asarray(tiles, dtype=np.uint32).reshape(grid, STAGES, ROWS, COLS)
    want_rec, want_tiles = healthy(grid, nonce)
    want_bad, want_tiles = injection_image(nonce, grid, inject)
    want_rec[:, REC_BAD:REC_BAD + STAGES] = want_bad
    bad = np.argwhere(til != want_tiles)
    assert bad.size == 0, (f"nonce {nonce:#x} grid {grid}: {len(bad)} tile words differ, first (wg, stage, i, j) "
                           f"{tuple(bad[0])}: got {int(til[tuple(bad[0])]):#010x} want "
                           f"{int(want_tiles[tuple(bad[0])]):#010x}")
    keep = [w for w in range(REC_WORDS) if w not in HW_WORDS]
    assert (rec[:, keep] == want_rec[:, keep]).all(), (nonce, grid, inject, rec[:, keep].tolist())
    assert (rec[:, REC_BAD:REC_BAD + STAGES] == want_bad).all(), (inject, rec[:, REC_BAD:REC_BAD + STAGES].tolist())
    assert (rec[:, REC_XCC] < 16).all(), rec[:, REC_XCC].tolist()
    assert (rec[:, REC_HWID:REC_HWID + WAVES] != 0).all(), rec[:, REC_HWID:REC_HWID + WAVES].tolist()


# ---- fault and wrong-kernel models (on the tile image) ------------------------------
def stuck_bit(tiles: np.ndarray, bit: int, value: int) -> np.ndarray:
    t = np.array(tiles, dtype=np.uint32)
    return t | np.uint32(1 << bit) if value else t & np.uint32(~(1 << bit) & M32)


def _tile_from(fn, nw: int, stage: int) -> list:
    a, b, c = operands(stage, nw)
    av = [[decode(w) for w in row] for row in a]
    bv = [[decode(w) for w in row] for row in b]
    cv = [[decode(w) for w in row] for row in c]
    out = []
    for i in range(ROWS):
        for j in range(COLS):
            v = fn(av, bv, cv, i, j)
            # a wrong kernel's value need not be exact or non-zero: any word that is not the right one will do
            out.append(encode(v) if v != 0 and is_normal(v) else 0)
    return out


def wrong_kernel_models(nonce: int, grid: int) -> dict:
    """Tile images of kernels that get the instruction's contract wrong."""
    good = tiles_image(nonce, grid)

    def rebuilt(fn):
        return np.array([[_tile_from(fn, wave_nonce(nonce, wg, 0), s) for s in range(STAGES)] for wg in range(grid)],
                        dtype=np.uint32).reshape(good.shape)
    half = np.array(good)
    for blk in range(0, ROWS, 8):                       # rows 8n..8n+3 belong to lanes 0-31, 8n+4..8n+7 to 32-63
        half[:, :, blk:blk + 4], half[:, :, blk + 4:blk + 8] = good[:, :, blk + 4:blk + 8], good[:, :, blk:blk + 4]
    return {
        "transposed store": np.ascontiguousarray(good.transpose(0, 1, 3, 2)),
        "k operands crossed": rebuilt(lambda a, b, c, i, j: c[i][j] + a[i][0] * b[1][j] + a[i][1] * b[0][j]),
        "second k term dropped": rebuilt(lambda a, b, c, i, j: c[i][j] + a[i][0] * b[0][j]),
        "C omitted": rebuilt(lambda a, b, c, i, j: a[i][0] * b[0][j] + a[i][1] * b[1][j]),
        "half-waves exchanged": half,
        "stages in another order": np.ascontiguousarray(good[:, ::-1]),
    }


# ---- the verdict (datapath_verify.h), from the field comments of mi355x_datapath_result ----
def verdict(records, tiles, grid: int, nonce: int) -> dict:
    rec = [[int(x) for x in row] for row in np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)]
    got = np.asarray(tiles, dtype=np.uint32).reshape(grid, WG_WORDS)
    want = tiles_image(nonce, grid).reshape(grid, WG_WORDS)
    present = [wg for wg, r in enumerate(rec)
               if r[REC_MAGIC] == MAGIC and r[REC_WG] == wg and r[REC_NONCE] == nonce ^ wg]
    stage_bad = [sum(rec[wg][REC_BAD + s] for wg in present) & M32 for s in range(STAGES)]
    wrong = {wg: np.flatnonzero(got[wg] != want[wg]) for wg in present}
    first = next(((wg, int(w[0])) for wg, w in wrong.items() if w.size), None)
    xccs = [rec[wg][REC_XCC] & 0xF for wg in present]
    cus = {(rec[wg][REC_XCC] & 0xF, rec[wg][REC_HWID] >> 8 & 0xFF) for wg in present}
    simds = {(rec[wg][REC_XCC] & 0xF, rec[wg][REC_HWID + v] >> 8 & 0xFF, rec[wg][REC_HWID + v] >> 4 & 0x3)
             for wg in present for v in range(WAVES)}
    records_ok = sum(1 for wg in present if not wrong[wg].size and not any(rec[wg][REC_BAD:REC_BAD + STAGES]))
    out = {
        "nonce": nonce, "grid": grid, "records_ok": records_ok,
        "mfma_bad": sum(sum(rec[wg][REC_BAD:REC_BAD + STAGES]) for wg in present) & M32,
        "stage_bad": stage_bad,
        "tile_bad": sum(int(w.size) for w in wrong.values()),
        "first_bad_wg": -1, "first_bad_stage": -1, "first_bad_word": -1,
        "first_bad_got": 0, "first_bad_want": 0, "first_bad_xor": 0,
        "cus_covered": len(cus), "simds_covered": len(simds), "xccs_covered": len(set(xccs)),
        "ok": records_ok == grid,
        "kfd_node_id": -1, "pci_bus_id": "",        # a verdict on records alone names no agent (hsa_chip.cpp does)
    }
    if first:
        wg, w = first
        g, e = int(got[wg][w]), int(want[wg][w])
        out.update(first_bad_wg=wg, first_bad_stage=w // TILE_WORDS, first_bad_word=w % TILE_WORDS,
                   first_bad_got=g, first_bad_want=e, first_bad_xor=g ^ e)
    return out


def assert_verdict(got: dict, want: dict, what: str = "") -> None:
    """`got`: a parsed datapath_json line; `want`: verdict(). Every field of
    `want` equal in type and value."""
    for key, w in want.items():
        assert key in got, f"{what}: no {key!r} in {sorted(got)}"
        assert type(got[key]) is type(w) and got[key] == w, f"{what}: {key} {got[key]!r} want {w!r}"


# ---- native/tests/datapath_contract_cli.cpp ------------------------------------------
RECORDS, TILES = 0, 1      # a patch's array


def compile_cli(exe, extra_flags=()) -> Path:
    from .contract_cli import host_compiler
    cxx = host_compiler()
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", *extra_flags]
    for inc in CLI_INCLUDES:
        cmd += ["-I", str(inc)]
    subprocess.run(cmd + [str(CLI_SOURCE), "-o", str(exe)], check=True, timeout=300)
    return Path(exe)


def contract_cli(build_dir) -> Path:
    """The program the native build left in the package's bin directory when it
    was built from the sources as they are now, else one compiled into `build_dir`."""
    from .. import _build
    from .contract_cli import host_compiler
    exe = _build.DATAPATH_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "datapath_contract_cli")


def case(records, tiles, grid: int, nonce: int, variants=()) -> bytes:
    """One `verdict` case; a variant is a list of (array, index, value) word replacements."""
    records = np.ascontiguousarray(records, dtype=np.uint32)
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
    assert records.size == grid * REC_WORDS and tiles.size == grid * WG_WORDS, (records.size, tiles.size, grid)
    blob = [struct.pack("<III", grid, nonce, len(variants)), records.tobytes(), tiles.tobytes()]
    for patches in variants:
        flat = np.asarray([tuple(int(x) & M32 for x in p) for p in patches], dtype=np.uint32).reshape(-1, 3)
        blob.append(struct.pack("<I", len(flat)) + flat.tobytes())
    return b"".join(blob)


def run_cli(cli, command: str, blob: bytes, expect: int, timeout: float = 300) -> list:
    r = subprocess.run([str(cli), command], input=blob, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    lines = r.stdout.decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == expect, (len(lines) - 1, expect)
    return lines[:-1]


def verdicts(cli, blobs, expect: int) -> list:
    return [json.loads(ln) for ln in run_cli(cli, "verdict", b"".join(blobs), expect)]
