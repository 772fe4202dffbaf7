"""Independent reference for the int8 MFMA datapath check
(mi355x_mfma_datapath_i8, native/src/health/datapath_i8_kernel.h,
datapath_i8_verify.h).

Written from the recipe in the header's comment, in Python integers: a
fragment is a list of signed bytes by position (block, dword, byte), a tile is
C plus the sum of byte products position by position. Nothing here can
overflow or round, and `overflow_margin` shows how far every output stays from
the int32 range under any summation order.

Also: the record / tile image a correct kernel writes, the verdict the host
draws from them, wrong-kernel and stuck-bit models, and a driver for
native/tests/datapath_i8_contract_cli.cpp.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
CLI_SOURCE = REPO / "native" / "tests" / "datapath_i8_contract_cli.cpp"
CLI_INCLUDES = (REPO / "native" / "include", REPO / "native" / "src" / "health")

M32 = 0xFFFFFFFF
STAGES = 5
DIM = (32, 32, 32, 32, 16)          # rows = columns of a stage's tile
BLOCKS = (2, 2, 2, 2, 4)            # K-blocks of a stage's instruction; a block is 4 dwords = 16 bytes
DWORDS = 4
TILE_WORDS = tuple(d * d for d in DIM)
TILE_OFFSET = (0, 1024, 2048, 3072, 4096)
WG_WORDS = 4 * 1024 + 256
REC_WORDS = 16
WAVES = 4
THREADS = 256
MAGIC = int.from_bytes(b"DPI8", "big")
REC_MAGIC, REC_WG, REC_NONCE, REC_XCC, REC_HWID, REC_BAD = 0, 1, 2, 3, 4, 8

GOLDEN, MURMUR = 0x9E3779B1, 0x85EBCA77
SEL_A, SEL_B, SEL_C, SEL_SIGN, SEL_ROT = 0x0000, 0x1000, 0x2000, 0x3000, 0x3800
ONE_HOT_A, ONE_HOT_B = (1,), (0,)   # the stages whose A / B operand is one-hot
ZERO_A = (3,)


# ---- integer hashes ---------------------------------------------------------------
def wave_nonce(nonce: int, wg: int, wave: int) -> int:
    return ((nonce ^ wg * GOLDEN & M32) + wave * MURMUR) & M32


def mix(nw: int, stage: int, selector: int) -> int:
    h = nw ^ ((stage + 0x11) * GOLDEN & M32) ^ (selector * MURMUR & M32)
    for shift, mult in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        h ^= h >> shift
        h = h * mult & M32
    return h ^ h >> 16


def signed32(word: int) -> int:
    return word - (1 << 32) if word >> 31 else word


def signed_bytes(word: int) -> list:
    """The four bytes of a word, low byte first, as signed integers."""
    return [(b ^ 0x80) - 0x80 for b in word.to_bytes(4, "little")]


# ---- operand words ------------------------------------------------------------------
def _any(nw: int, stage: int, selector: int, rc: int, block: int, dword: int) -> int:
    """Any bytes; dword 1 is the complement of dword 0, dword 3 of dword 2."""
    h = mix(nw, stage, selector + (rc * 4 + block) * 4 + dword // 2 * 2)
    return h ^ M32 if dword % 2 else h


def onehot_position(stage: int, rc: int, nw: int) -> int:
    """The one of the 32 (block, dword, byte) positions where row / column `rc`
    of a one-hot operand is not zero."""
    return (rc + mix(nw, stage, SEL_ROT) % 32) % 32


def _onehot(nw: int, stage: int, rc: int, block: int, dword: int) -> int:
    pos = onehot_position(stage, rc, nw)
    if pos // 4 != block * DWORDS + dword:
        return 0
    byte = 0xFF if mix(nw, stage, SEL_SIGN + rc) >> 31 else 0x01
    return byte << 8 * (pos % 4)


def a_word(stage: int, row: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_A:
        return _onehot(nw, stage, row, block, dword)
    if stage in ZERO_A:
        return 0
    return _any(nw, stage, SEL_A, row, block, dword)


def b_word(stage: int, col: int, block: int, dword: int, nw: int) -> int:
    if stage in ONE_HOT_B:
        return _onehot(nw, stage, col, block, dword)
    return _any(nw, stage, SEL_B, col, block, dword)


def c_word(stage: int, row: int, col: int, nw: int) -> int:
    if stage in (2, 4):
        return (signed32(mix(nw, stage, SEL_C + 32 * row + col)) >> 1) & M32    # arithmetic shift
    if stage == 3:
        h = mix(nw, 3, SEL_C + 32 * row + (0 if col == 1 else col))
        return h ^ M32 if col == 1 else h
    return 0


@lru_cache(maxsize=None)
def operands(stage: int, nw: int):
    """(A words [dim][blocks*4], B words [dim][blocks*4], C words [dim][dim]) of one
    wave's stage; operand word block*4 + dword of a row / column."""
    dim, words = DIM[stage], BLOCKS[stage] * DWORDS
    a = tuple(tuple(a_word(stage, i, w // 4, w % 4, nw) for w in range(words)) for i in range(dim))
    b = tuple(tuple(b_word(stage, j, w // 4, w % 4, nw) for w in range(words)) for j in range(dim))
    c = tuple(tuple(c_word(stage, i, j, nw) for j in range(dim)) for i in range(dim))
    return a, b, c


def _bytes_of(fragment) -> list:
    return [v for word in fragment for v in signed_bytes(word)]


@lru_cache(maxsize=None)
def expected_tile(stage: int, nw: int) -> tuple:
    """The output words of one wave's stage, row-major: C + sum over positions
    of A byte times B byte, in Python integers."""
    a, b, c = operands(stage, nw)
    av, bv = [_bytes_of(f) for f in a], [_bytes_of(f) for f in b]
    dim = DIM[stage]
    out = []
    for i in range(dim):
        for j in range(dim):
            d = signed32(c[i][j]) + sum(x * y for x, y in zip(av[i], bv[j]))
            assert -(1 << 31) <= d < 1 << 31, (stage, i, j, d)
            out.append(d & M32)
    return tuple(out)


def overflow_margin(stage: int, nw: int) -> int:
    """max over the stage's outputs of |C| + sum |a|*|b|: no partial sum, in any
    order, can be larger in magnitude."""
    a, b, c = operands(stage, nw)
    av, bv = [[abs(v) for v in _bytes_of(f)] for f in a], [[abs(v) for v in _bytes_of(f)] for f in b]
    dim = DIM[stage]
    return max(abs(signed32(c[i][j])) + sum(x * y for x, y in zip(av[i], bv[j]))
               for i in range(dim) for j in range(dim))


def _both(words) -> int:
    ones = zeros = 0
    for w in words:
        ones, zeros = ones | w, zeros | (w ^ M32)
    return ones & zeros


def toggle_masks(nw: int) -> dict:
    """Per operand, the bits that take both values: in every single fragment
    (the four dwords one lane hands the instruction) of A in stage 0 and of B
    in stage 1, in every row of C in stage 3, and in every row of D in stage 3."""
    a0, _, _ = operands(0, nw)
    _, b1, _ = operands(1, nw)
    _, _, c3 = operands(3, nw)
    d3 = expected_tile(3, nw)
    def every(groups) -> int:
        out = M32
        for g in groups:
            out &= _both(g)
        return out

    def fragments(rows) -> list:
        return [row[4 * h:4 * h + 4] for row in rows for h in range(len(row) // 4)]
    return {"A": every(fragments(a0)), "B": every(fragments(b1)), "C": every(c3),
            "D": every(d3[32 * i:32 * i + 32] for i in range(32))}


def selected_positions(stage: int, nw: int) -> list:
    """Stage 0 / 1: per column / row, the fragment position its one-hot byte
    selects, read back from the operand words (not from onehot_position)."""
    a, b, _ = operands(stage, nw)
    frags = b if stage in ONE_HOT_B else a
    out = []
    for f in frags:
        nz = [p for p, v in enumerate(_bytes_of(f)) if v]
        assert len(nz) == 1 and _bytes_of(f)[nz[0]] in (1, -1), (stage, f)
        out.append(nz[0])
    return out


# ---- what a correct kernel writes ----------------------------------------------------
_tiles_cache: dict = {}


def tiles_image(nonce: int, grid: int) -> np.ndarray:
    """tiles[wg][4352] as uint32: wave 0's five tiles of every workgroup, four
    of 32x32 and one of 16x16. Computed once per (nonce, grid) and read-only:
    copy before changing it."""
    key = (nonce, grid)
    if key not in _tiles_cache:
        t = np.array([[w for s in range(STAGES) for w in expected_tile(s, wave_nonce(nonce, wg, 0))]
                      for wg in range(grid)], dtype=np.uint32).reshape(grid, WG_WORDS)
        t.setflags(write=False)
        _tiles_cache[key] = t
    return _tiles_cache[key]


def spread_placement(grid: int, xcds: int = 8) -> list:
    """(xcc, cu-bits) per workgroup: dealt round-robin to the XCDs."""
    return [(wg % xcds, wg // xcds) for wg in range(grid)]


def healthy(grid: int, nonce: int, placement=None):
    """(records, tiles) a correct mi355x_mfma_datapath_i8 would write; wave v of
    a workgroup on SIMD v of its CU."""
    placement = list(placement or spread_placement(grid))
    assert len(placement) == grid
    recs = np.zeros((grid, REC_WORDS), dtype=np.uint32)
    for wg, (xcc, cu) in enumerate(placement):
        recs[wg, REC_MAGIC], recs[wg, REC_WG], recs[wg, REC_NONCE], recs[wg, REC_XCC] = MAGIC, wg, nonce ^ wg, xcc
        for v in range(WAVES):
            recs[wg, REC_HWID + v] = cu << 8 | v << 4 | 0x1
    return recs, tiles_image(nonce, grid).copy()


ACC_REGS = (16, 16, 16, 16, 4)
INDEX_STRIDE = 16                   # inject index = stage * 16 + register


def accumulator_element(stage: int, lane: int, reg: int) -> tuple:
    """(row, column) of the stage's tile that accumulator register `reg` of lane
    `lane` holds: 32x32: D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]; 16x16: D[4*(l>>4) + r][l&15]."""
    assert 0 <= lane < 64 and 0 <= reg < ACC_REGS[stage]
    if DIM[stage] == 16:
        return 4 * (lane >> 4) + reg, lane & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


def injection_image(nonce: int, grid: int, inject=None) -> tuple:
    """(stage_bad (grid, 5), tiles (grid, 4352) uint32) that
    mi355x_mfma_datapath_i8 of the test-only build must leave behind under
    `inject` (a raw_kernels request's "inject" object: index = stage * 16 +
    register; None for the hook off), from the documented layout alone. The
    wrong word is counted once, by its workgroup, in its stage's counter; it
    reaches the host's tiles only from wave 0, and there it differs from the
    healthy word by exactly the mask. An index that names no register injects nothing."""
    stage_bad = np.zeros((grid, STAGES), dtype=np.int64)
    tiles = tiles_image(nonce, grid).copy()
    if inject is not None and inject["mask"] & M32 and inject["wg"] < grid:
        assert inject["kind"] == "mfma", inject
        wg, wave, lane, index = inject["wg"], inject["wave"], inject["lane"], inject["index"]
        stage, reg = divmod(index, INDEX_STRIDE)
        if wave < WAVES and lane < 64 and stage < STAGES and reg < ACC_REGS[stage]:
            stage_bad[wg, stage] = 1
            if wave == 0:
                i, j = accumulator_element(stage, lane, reg)
                tiles[wg, TILE_OFFSET[stage] + i * DIM[stage] + j] ^= np.uint32(inject["mask"] & M32)
    return stage_bad, tiles


HW_WORDS = (REC_XCC, REC_HWID, REC_HWID + 1, REC_HWID + 2, REC_HWID + 3)   # hardware's, not the reference's


def check_raw(records, tiles, nonce: int, grid: int, inject=None) -> None:
    """Every word the kernel wrote against the reference image: the whole tile
    buffer, and the records but for where the workgroup ran (those: XCC id in
    range, HW_ID words non-zero). `inject`: the injection the test-only build
    was asked for (injection_image)."""
    rec = np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)
    til = np.asarray(tiles, dtype=np.uint32).reshape(grid, WG_WORDS)
    want_rec, _ = healthy(grid, nonce)
    want_bad, want_tiles = injection_image(nonce, grid, inject)
    want_rec[:, REC_BAD:REC_BAD + STAGES] = want_bad
    bad = np.argwhere(til != want_tiles)
    if bad.size:
        wg, w = (int(x) for x in bad[0])
        stage = max(s for s in range(STAGES) if TILE_OFFSET[s] <= w)
        raise AssertionError(f"nonce {nonce:#x} grid {grid}: {len(bad)} tile words differ, first wg {wg} stage {stage} "
                             f"word {w - TILE_OFFSET[stage]}: got {int(til[wg, w]):#010x} want "
                             f"{int(want_tiles[wg, w]):#010x}")
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
    """A tile from `fn(a_words, b_words, c, stage) -> int` per element, wrapped to 32 bits."""
    a, b, c = operands(stage, nw)
    dim = DIM[stage]
    return [fn(a[i], b[j], signed32(c[i][j]), stage) & M32 for i in range(dim) for j in range(dim)]


def _dot(a_words, b_words, sext=True) -> int:
    total = 0
    for x, y in zip(a_words, b_words):
        xs = signed_bytes(x) if sext else list(x.to_bytes(4, "little"))
        ys = signed_bytes(y) if sext else list(y.to_bytes(4, "little"))
        total += sum(p * q for p, q in zip(xs, ys))
    return total


def _blocks_swapped(words) -> list:
    blocks = [words[k:k + 4] for k in range(0, len(words), 4)]
    return [w for blk in reversed(blocks) for w in blk]


def _dwords_reversed(words) -> list:
    return [w for k in range(0, len(words), 4) for w in reversed(words[k:k + 4])]


def wrong_kernel_models(nonce: int, grid: int) -> dict:
    """Tile images of kernels (or of a reference) that get the instruction's
    contract wrong."""
    good = tiles_image(nonce, grid)

    def rebuilt(fn):
        return np.array([[w for s in range(STAGES) for w in _tile_from(fn, wave_nonce(nonce, wg, 0), s)]
                         for wg in range(grid)], dtype=np.uint32).reshape(good.shape)

    transposed = np.array(good)
    for s in range(STAGES):
        dim, off = DIM[s], TILE_OFFSET[s]
        transposed[:, off:off + dim * dim] = good[:, off:off + dim * dim].reshape(grid, dim, dim) \
            .transpose(0, 2, 1).reshape(grid, dim * dim)
    # the 16x16 tile stored as if its registers lay as in the 32x32 form: register r of lane l goes to row
    # r + 4 * (l >> 5) (the 32x32 formula for r < 4), column l & 15; rows never written keep the buffer's fill
    wrong16 = np.array(good)
    t16 = good[:, TILE_OFFSET[4]:].reshape(grid, 16, 16)
    w16 = np.full((grid, 16, 16), M32, dtype=np.uint32)
    for lane in range(64):
        for reg in range(4):
            i, j = accumulator_element(4, lane, reg)
            w16[:, (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 15] = t16[:, i, j]
    wrong16[:, TILE_OFFSET[4]:] = w16.reshape(grid, 256)
    return {
        "A's K-blocks swapped against B's": rebuilt(lambda a, b, c, s: c + _dot(_blocks_swapped(a), b)),
        "dwords of A reversed within a block": rebuilt(lambda a, b, c, s: c + _dot(_dwords_reversed(a), b)),
        "transposed store": transposed,
        "C dropped": rebuilt(lambda a, b, c, s: _dot(a, b)),
        "bytes unsigned": rebuilt(lambda a, b, c, s: c + _dot(a, b, sext=False)),
        "16x16 tile stored with the 32x32 row formula": wrong16,
    }


# ---- the verdict (datapath_i8_verify.h), from the field comments of mi355x_datapath_i8_result ----
def verdict(records, tiles, grid: int, nonce: int) -> dict:
    rec = [[int(x) for x in row] for row in np.asarray(records, dtype=np.uint32).reshape(grid, REC_WORDS)]
    got = np.asarray(tiles, dtype=np.uint32).reshape(grid, WG_WORDS)
    want = tiles_image(nonce, grid)
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
        stage = max(s for s in range(STAGES) if TILE_OFFSET[s] <= w)
        g, e = int(got[wg][w]), int(want[wg][w])
        out.update(first_bad_wg=wg, first_bad_stage=stage, first_bad_word=w - TILE_OFFSET[stage],
                   first_bad_got=g, first_bad_want=e, first_bad_xor=g ^ e)
    return out


def assert_verdict(got: dict, want: dict, what: str = "") -> None:
    """`got`: a parsed datapath_i8_json line; `want`: verdict(). Every field of
    `want` equal in type and value."""
    for key, w in want.items():
        assert key in got, f"{what}: no {key!r} in {sorted(got)}"
        assert type(got[key]) is type(w) and got[key] == w, f"{what}: {key} {got[key]!r} want {w!r}"


# ---- native/tests/datapath_i8_contract_cli.cpp ----------------------------------------
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
    exe = _build.DATAPATH_I8_CLI
    if os.access(exe, os.X_OK) and (_build._up_to_date([exe]) or not host_compiler()):
        return exe
    return compile_cli(Path(build_dir) / "datapath_i8_contract_cli")


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
