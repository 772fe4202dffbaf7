"""datapath_f16_kernel.h and datapath_f16_verify.h against the independent
reference (testing/datapath_f16_reference.py), CPU only, through the host-only
program native/tests/datapath_f16_contract_cli.cpp: the operand words and the
seven expected tiles word for word, at grids 1 and 3 and two nonces the whole image, the argument structs (production and
inject builds) against their ctypes mirrors, the shipped verdict on the
reference image with stuck bits, single flips, wrong-kernel models, wrong
records and truncated input; and the serve grammar of the request, in the server's own parser
(probe_contract_cli parse) and against the stub probe."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_f16_reference as db
from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import datapath_i8_reference as d8
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import raw_kernels

GRID = 3
NONCE = 0xDEADBEEF
FLIP_BITS = (0, 7, 8, 19, 30, 31)
STUB = os.path.join(os.path.dirname(raw_kernels.__file__), "stub_probe.py")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return db.contract_cli(tmp_path_factory.mktemp("datapath_f16_contract"))


def _gen(cli, lines):
    r = subprocess.run([str(cli), "gen"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def test_operand_words_and_tiles_agree_with_header_word_for_word(cli):
    lines, want = [], []
    for n in dp.NONCES:
        for wg, wave in dp.WG_WAVES + ((0x3FFFFFFF, 2), (0x40000000, 3)):
            lines.append(f"wave_nonce {n} {wg} {wave}")
            want.append([db.wave_nonce(n, wg, wave)])
        for wg, wave in dp.WG_WAVES:
            nw = db.wave_nonce(n, wg, wave)
            for stage in range(db.STAGES):
                a, b, c = db.operands(stage, nw)
                dim, dw = db.DIM[stage], db.DWORDS[stage]
                for rc in range(dim):
                    for w in range(db.BLOCKS[stage] * dw):
                        lines.append(f"a {stage} {rc} {w // dw} {w % dw} {nw}")
                        want.append([a[rc][w]])
                        lines.append(f"b {stage} {rc} {w // dw} {w % dw} {nw}")
                        want.append([b[rc][w]])
                for i in range(dim):
                    for j in range(dim):
                        lines.append(f"c {stage} {i} {j} {nw}")
                        want.append([c[i][j]])
                lines.append(f"tile {stage} {nw}")
                want.append(list(db.expected_tile(stage, nw)))
    got = _gen(cli, lines)
    for ln, g, w in zip(lines, got, want):
        assert g == w, ln


@pytest.mark.parametrize("grid", (1, 3))
@pytest.mark.parametrize("nonce", (0xFFFFFFFF, NONCE))
def test_header_image_equals_the_reference_image(cli, grid, nonce):
    """Wave 0's seven tiles of every workgroup, as datapath_f16_verify.h expects them."""
    assert (db.header_tiles(cli, nonce, grid) == db.tiles_image(nonce, grid)).all()


def test_gen_refuses_what_the_recipe_does_not_define(cli):
    for bad in ("a 7 0 0 0 1", "a 0 32 0 0 1", "a 0 0 2 0 1", "a 4 16 0 0 1", "b 6 16 0 0 1", "a 0 0 0 4 1",
                "a 5 0 0 2 1", "b 6 0 4 0 1", "a 6 0 0 2 1", "c 4 0 16 1", "c 6 16 0 1", "tile 7 1", "scale 4 0 0 0 1"):
        r = subprocess.run([str(cli), "gen"], input=bad + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, bad


def _layout(exe, command):
    r = subprocess.run([str(exe), command], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    structs, defines = {}, {}
    for ln in r.stdout.splitlines():
        s, f, v = ln.split()
        if s == "define":
            defines[f] = int(v)
        else:
            structs.setdefault(s, []).append((f, int(v)))
    return structs, defines


def _mirror(structs: dict) -> dict:
    return {name: [(f, getattr(cls, f).offset) for f, _ in cls._fields_] + [("sizeof", ctypes.sizeof(cls))]
            for name, cls in structs.items()}


def test_layout_equals_the_ctypes_mirror_and_the_reference_constants(cli):
    structs, defines = _layout(cli, "layout")
    assert structs == _mirror(raw_kernels.DATAPATH_F16_ARG_STRUCTS)
    assert dict(structs["mi355x_datapath_f16_args"])["sizeof"] == 24
    # the dicts that mirror the other headers keep their contents
    assert sorted(raw_kernels.ARG_STRUCTS) == ["mi355x_burn_args", "mi355x_hbm_args", "mi355x_liveness_args",
                                               "mi355x_sweep_args"]
    assert list(raw_kernels.DATAPATH_ARG_STRUCTS) == ["mi355x_datapath_args"]
    assert list(raw_kernels.INJECT_ARG_STRUCTS) == ["mi355x_sweep_args"]
    assert list(raw_kernels.DATAPATH_INJECT_ARG_STRUCTS) == ["mi355x_datapath_args"]
    assert raw_kernels.DATAPATH_F16_WG_WORDS == db.WG_WORDS
    assert defines == {"MI355X_DPHF_THREADS": db.THREADS, "MI355X_DPHF_STAGES": db.STAGES,
                       "MI355X_DPHF_TILE": 1024, "MI355X_DPHF_TILE16": 256,
                       "MI355X_DPHF_WG_WORDS": db.WG_WORDS, "MI355X_DPHF_REC_WORDS": db.REC_WORDS,
                       "MI355X_DPHF_MAGIC": db.MAGIC, "MI355X_DPHFREC_MAGIC": db.REC_MAGIC,
                       "MI355X_DPHFREC_WG": db.REC_WG, "MI355X_DPHFREC_NONCE": db.REC_NONCE,
                       "MI355X_DPHFREC_XCC": db.REC_XCC, "MI355X_DPHFREC_HWID": db.REC_HWID,
                       "MI355X_DPHFREC_BAD": db.REC_BAD}
    assert len({db.MAGIC, dp.MAGIC, d8.MAGIC}) == 3 and db.MAGIC == 0x44504846
    assert list(raw_kernels.DATAPATH_I8_ARG_STRUCTS) == ["mi355x_datapath_i8_args"]


def test_args_of_the_inject_build_equal_the_ctypes_mirror(cli, tmp_path):
    """The header compiled as the test-only code object is: with MI355X_TEST_INJECT."""
    exe = db.compile_cli(tmp_path / "datapath_f16_contract_cli_inject", ("-DMI355X_TEST_INJECT=1",))
    structs, defines = _layout(exe, "inject-layout")
    assert structs == _mirror(raw_kernels.DATAPATH_F16_INJECT_ARG_STRUCTS)
    assert dict(structs["mi355x_datapath_f16_args"])["sizeof"] == 48
    prod = _mirror({"mi355x_datapath_f16_args": raw_kernels.DatapathF16Args})["mi355x_datapath_f16_args"][:-1]
    assert structs["mi355x_datapath_f16_args"][:len(prod)] == prod     # the extension only trails
    assert defines == {"MI355X_DPHF_INJECT_NONE": raw_kernels.INJECT_KINDS["none"],
                       "MI355X_DPHF_INJECT_MFMA": raw_kernels.INJECT_KINDS["mfma"]}
    # without the macro `inject-layout` prints no struct
    structs, defines = _layout(cli, "inject-layout")
    assert structs == {} and defines


def test_launcher_plans_the_request_and_packs_the_injection_words(tmp_path):
    ptrs = {"records": 0x1000, "tiles": 0x2000}
    base = {"id": "x", "kernel": "datapath_f16", "nonce": 7, "grid": 2}
    bufs, make, wgs = raw_kernels.plan(base, tmp_path)
    assert type(make(ptrs)) is raw_kernels.DatapathF16Args and wgs == 2
    assert [(n, len(b)) for n, _, b in bufs] == [("records", 2 * 16 * 4), ("tiles", 2 * db.WG_WORDS * 4)]
    assert raw_kernels.KERNELS["datapath_f16"] == ("mi355x_mfma_datapath_f16", 256)
    off = raw_kernels.plan(dict(base, code_object="inject"), tmp_path)[1](ptrs)
    assert type(off) is raw_kernels.DatapathF16InjectArgs and off.inject_kind == 0 and off.inject_mask == 0
    inj = {"kind": "mfma", "wg": 1, "wave": 3, "lane": 63, "index": 67, "mask": 1 << 31}
    a = raw_kernels.plan(dict(base, code_object="inject", inject=inj), tmp_path)[1](ptrs)
    assert (a.inject_kind, a.inject_wg, a.inject_wave, a.inject_lane, a.inject_index, a.inject_mask) == \
        (1, 1, 3, 63, 67, 1 << 31)
    assert (a.records, a.tiles, a.nonce, a.grid) == (0x1000, 0x2000, 7, 2)
    for bad in (dict(base, inject=inj), dict(base, code_object="inject", inject=dict(inj, kind="lds"))):
        with pytest.raises(ValueError):
            raw_kernels.plan(bad, tmp_path)[1](ptrs)


# ---- the shipped verdict -------------------------------------------------------------------------
def _patches(good, changed):
    """The word replacements that turn the tile image `good` into `changed`."""
    g, c = np.asarray(good).ravel(), np.asarray(changed).ravel()
    return [(db.TILES, int(i), int(c[i])) for i in np.flatnonzero(g != c)]


def _apply(recs, tiles, patches):
    arrays = [np.array(recs, dtype=np.uint32).ravel(), np.array(tiles, dtype=np.uint32).ravel()]
    for arr, idx, val in patches:
        arrays[arr][idx] = val & 0xFFFFFFFF
    return arrays


def _check(cli, recs, tiles, grid, nonce, variants):
    """Every variant through the shipped verdict, each equal to the reference verdict field by field."""
    names = list(variants)
    got = db.verdicts(cli, [db.case(recs, tiles, grid, nonce, [variants[n] for n in names])], 1 + len(names))
    db.assert_verdict(got[0], db.verdict(recs, tiles, grid, nonce), "as given")
    out = {}
    for name, g in zip(names, got[1:]):
        r, t = _apply(recs, tiles, variants[name])
        db.assert_verdict(g, db.verdict(r, t, grid, nonce), str(name))
        out[name] = g
    return got[0], out


@pytest.mark.parametrize("nonce", dp.NONCES)
def test_healthy_image_passes_and_reports_coverage(cli, nonce):
    recs, tiles = db.healthy(GRID, nonce, placement=[(0, 5), (1, 5), (1, 6)])
    good, _ = _check(cli, recs, tiles, GRID, nonce, {})
    assert good["ok"] is True and good["records_ok"] == GRID and good["tile_bad"] == 0 and good["error"] == ""
    assert (good["cus_covered"], good["simds_covered"], good["xccs_covered"]) == (3, 12, 2)
    assert good["first_bad_stage"] == -1 and good["first_bad_xor"] == 0
    assert good["stage_bad"] == [0] * 7 and good["mfma_bad"] == 0


def test_every_stuck_bit_fails_the_shipped_verdict(cli):
    recs, tiles = db.healthy(GRID, NONCE)
    variants = {(bit, value): _patches(tiles, db.stuck_bit(tiles, bit, value)) for bit in range(32) for value in (0, 1)}
    # Every sum is an odd number of quanta below 2^23 and the one-hot stages' products have at most 22
    # significant bits, so an f32 significand holds them shifted left by one or more: bit 0 of D is never
    # set, and bit 1 only by a sum of 2^22 quanta or more, which 16 or 32 mixed-sign terms of this image do
    # not reach. Stuck at 0 there is the f32 and bf16 checks' C-in -> D-out stage; every other stuck bit of D,
    # those two stuck at 1 included, changes some word.
    unseen = {k for k, v in variants.items() if not v}
    assert {(0, 0)} <= unseen <= {(0, 0), (1, 0)}
    variants = {k: v for k, v in variants.items() if k not in unseen}
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for (bit, value), g in got.items():
        assert g["ok"] is False and g["tile_bad"] > 0 and g["first_bad_xor"] == 1 << bit, (bit, value, g)
        assert f"(bit {bit})" in g["error"]


@pytest.mark.parametrize("stage", range(db.STAGES))
def test_one_flipped_bit_is_one_bad_word_with_its_xor(cli, stage):
    recs, tiles = db.healthy(GRID, NONCE)
    flat = tiles.ravel()
    wg = GRID - 1
    variants = {}
    for k, bit in enumerate(FLIP_BITS):
        word = (k * 211 + 37 * stage + 5) % db.TILE_WORDS[stage]
        idx = wg * db.WG_WORDS + db.TILE_OFFSET[stage] + word
        variants[(bit, word)] = [(db.TILES, idx, int(flat[idx]) ^ 1 << bit)]
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for (bit, word), g in got.items():
        assert g["ok"] is False and g["tile_bad"] == 1 and g["records_ok"] == GRID - 1
        assert g["first_bad_xor"] == 1 << bit
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word)
        assert f"wg {wg} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in g["error"]


@pytest.mark.parametrize("stage", range(db.STAGES))
def test_first_and_last_word_of_a_stage_bits_0_and_31(cli, stage):
    recs, tiles = db.healthy(GRID, NONCE)
    flat = tiles.ravel()
    variants = {}
    for wg in (0, GRID - 1):
        for word in (0, db.TILE_WORDS[stage] - 1):
            for bit in (0, 31):
                idx = wg * db.WG_WORDS + db.TILE_OFFSET[stage] + word
                variants[(wg, word, bit)] = [(db.TILES, idx, int(flat[idx]) ^ 1 << bit)]
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for (wg, word, bit), g in got.items():
        assert g["ok"] is False and g["tile_bad"] == 1 and g["first_bad_xor"] == 1 << bit
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word)
        assert g["error"] == (f"{GRID - 1}/{GRID} workgroups exact (device_bad=0 tile_bad=1); first bad: wg {wg} "
                              f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})")


def test_last_word_of_the_16x16_tile_is_checked(cli):
    recs, tiles = db.healthy(GRID, NONCE)
    idx = GRID * db.WG_WORDS - 1
    _, got = _check(cli, recs, tiles, GRID, NONCE, {"last": [(db.TILES, idx, int(tiles.ravel()[idx]) ^ 2)]})
    g = got["last"]
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"], g["first_bad_xor"]) == (GRID - 1, 6, 255, 2)


def test_wrong_kernel_models_fail(cli):
    recs, tiles = db.healthy(GRID, NONCE)
    models = db.wrong_kernel_models(NONCE, GRID)
    assert len(models) == 11
    _, got = _check(cli, recs, tiles, GRID, NONCE, {n: _patches(tiles, t) for n, t in models.items()})
    for name, g in got.items():
        assert g["ok"] is False and g["records_ok"] == 0 and g["tile_bad"] > 100, (name, g)


def test_wrong_records_fail(cli):
    recs, tiles = db.healthy(GRID, NONCE)
    r = lambda wg, word, value: [(db.RECORDS, wg * db.REC_WORDS + word, value)]   # noqa: E731
    variants = {
        "missing record": r(1, db.REC_MAGIC, 0),
        "the f32 check's magic": r(1, db.REC_MAGIC, dp.MAGIC),
        "the int8 check's magic": r(2, db.REC_MAGIC, d8.MAGIC),
        "another workgroup's record": r(1, db.REC_WG, 2),
        "wrong echoed nonce": r(2, db.REC_NONCE, (NONCE ^ 2) + 1),
        "device bad count, stage 0": r(0, db.REC_BAD, 1),
        "device bad count, stage 4": r(0, db.REC_BAD + 4, 7),
    }
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for name, g in got.items():
        assert g["ok"] is False and g["records_ok"] == GRID - 1 and g["tile_bad"] == 0, (name, g)
        assert g["error"].startswith(f"{GRID - 1}/{GRID} workgroups exact")
    assert got["device bad count, stage 4"]["stage_bad"] == [0, 0, 0, 0, 7, 0, 0]
    assert got["device bad count, stage 4"]["mfma_bad"] == 7
    # an absent record counts for nothing: its tile is not looked at either
    both = variants["missing record"] + [(db.TILES, db.WG_WORDS + 9, 0)]
    _, got = _check(cli, recs, tiles, GRID, NONCE, {"missing, tile wrong too": both})
    assert got["missing, tile wrong too"]["tile_bad"] == 0


def test_unwritten_buffers_fail(cli):
    """What the host prefills (records 0, tiles 0xFF) is no verdict."""
    recs = np.zeros((GRID, db.REC_WORDS), dtype=np.uint32)
    tiles = np.full(GRID * db.WG_WORDS, 0xFFFFFFFF, dtype=np.uint32)
    good, _ = _check(cli, recs, tiles, GRID, NONCE, {})
    assert good["ok"] is False and good["records_ok"] == 0


def test_truncated_input_is_refused_and_yields_no_verdict(cli):
    recs, tiles = db.healthy(1, NONCE)
    blob = db.case(recs, tiles, 1, NONCE)
    for cut in (5, 12 + 16 * 4 - 1, len(blob) - 4, len(blob) - 1):
        r = subprocess.run([str(cli), "verdict"], input=blob[:cut], capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stdout == b"" and b"truncated" in r.stderr, cut
    # a variant cut short: the case as given is judged, the variant is refused
    whole = db.case(recs, tiles, 1, NONCE, [[(db.TILES, 0, 1)]])
    r = subprocess.run([str(cli), "verdict"], input=whole[:-4], capture_output=True, timeout=60)
    assert r.returncode == 2 and len(r.stdout.splitlines()) == 1 and json.loads(r.stdout)["ok"] is True
    # and a grid the check cannot have
    r = subprocess.run([str(cli), "verdict"], input=b"\0" * 12, capture_output=True, timeout=60)
    assert r.returncode == 2 and r.stdout == b""


# ---- the request against the stub probe -----------------------------------------------------------
OTHERS = ["probe 4 5 0:101", "sweep 4 5 0:102", "perf 64 5 64 0:103", "datapath 5 0:104", "datapath_i8 5 0:108",
          "@9 probe 4 5 1:109"]
F16 = ["datapath_f16 5 0:105", "@7 datapath_f16 5 0:106:2.5 3:107"]
GRAMMAR = [
    "datapath_f16 10 0:1", "@4 datapath_f16 10 0:1", "@18446744073709551615 datapath_f16 9.5 0:1:2.5 3:0x10",
    "datapath_f16 10", "datapath_f16 10 0:1 \r\n",
    # refused: the near-misses, and what refuses every kind
    "datapath_f1610 0:1", "datapath_f1610", "datapath _f16 10 0:1", "datapath_f1 10 0:1", "datapath_f16", "datapath_f16 ",
    "datapath_f16 x 0:1", "datapath_f16 10 0:1 x", "DATAPATH_F16 10 0:1", "@7datapath_f16 10 0:1", "datapath_f16_ 10 0:1",
    # the siblings are not mistaken for it, nor it for them
    "datapath 10 0:1", "datapath_i8 10 0:1", "datapath_bf16 10 0:6", "datapath_i16 10 0:1",
]


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    from rocm_k8s_device_plugin_amd.testing import stub_probe
    real = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), GRAMMAR)
    by_line = dict(zip(GRAMMAR, real))
    for line, r in by_line.items():
        assert stub_probe._parse(line) == r, line
    assert by_line["datapath_f16 10 0:1"] == {"tagged": False, "id": 0, "kind": "datapath_f16", "iters": 0,
                                               "timeout": 10, "mib": 0, "devices": [[0, 1, 10]]}
    assert by_line["@4 datapath_f16 10 0:1"] == {**by_line["datapath_f16 10 0:1"], "tagged": True, "id": 4}
    big = by_line["@18446744073709551615 datapath_f16 9.5 0:1:2.5 3:0x10"]
    assert big["id"] == 2 ** 64 - 1 and big["devices"] == [[0, 1, 2.5], [3, 16, 9.5]]
    assert by_line["datapath_f16 10"]["devices"] == [] and by_line["datapath_f16 10 0:1 \r\n"]["devices"] == [[0, 1, 10]]
    for line in GRAMMAR[5:16]:
        assert by_line[line] == "bad request", line
    assert [by_line[ln]["kind"] for ln in GRAMMAR[16:19]] == ["datapath", "datapath_i8", "datapath_bf16"]
    assert by_line["datapath_i16 10 0:1"] == "bad request"


def _serve(tmp_path, name, lines, control=None):
    ctl = tmp_path / f"{name}.json"
    ctl.write_text(json.dumps(control or {}))
    log = tmp_path / f"{name}.log"
    out = []
    p = subprocess.Popen([sys.executable, STUB, "--serve", "--keep"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                         text=True, env=dict(os.environ, MI355X_STUB_PROBE_CONTROL=str(ctl),
                                             MI355X_STUB_PROBE_LOG=str(log)))
    try:
        out.append(json.loads(p.stdout.readline()))
        for ln in lines:                             # one at a time: a tagged reply cannot overtake
            p.stdin.write(ln + "\n")
            p.stdin.flush()
            out.append(json.loads(p.stdout.readline()))
        p.stdin.write("quit\n")
        p.stdin.flush()
        assert p.wait(timeout=20) == 0
    finally:
        if p.poll() is None:
            p.kill()
    return out, log.read_text().split()


def _masked(doc):
    return {k: v for k, v in doc.items() if not k.startswith("t_")}


def test_serve_grammar_and_the_other_replies_stay_as_they_were(tmp_path):
    with_f16, log = _serve(tmp_path, "with", OTHERS[:2] + F16[:1] + OTHERS[2:4] + F16[1:] + OTHERS[4:])
    without, log0 = _serve(tmp_path, "without", OTHERS)
    hello, probe, sweep, untagged, perf, f32, tagged, i8, probe9 = with_f16
    assert [_masked(d) for d in (hello, probe, sweep, perf, f32, i8, probe9)] == [_masked(d) for d in without]
    for doc in (hello, probe, sweep, perf, f32, i8, probe9):
        assert "datapath_f16" not in doc and "datapath_f16" not in json.dumps(doc)
    assert f32["datapath"] is True and i8["datapath_i8"] is True
    assert untagged["datapath_f16"] is True and "id" not in untagged and "datapath" not in untagged
    assert "datapath_i8" not in untagged
    d = untagged["devices"][0]
    assert untagged["ok"] is True and d["ok"] is True and d["nonce"] == 105 and d["ordinal"] == 0
    assert d["stage_bad"] == [0] * 7 and d["records_ok"] == d["grid"] and d["kept_queue"] is True
    assert tagged["id"] == 7 and tagged["datapath_f16"] is True
    assert [(x["ordinal"], x["nonce"]) for x in tagged["devices"]] == [(0, 106), (3, 107)]
    assert [ln for ln in log if ln.startswith("datapath_f16:")] == ["datapath_f16:0", "datapath_f16:0", "datapath_f16:3"]
    assert [ln for ln in log if ln.startswith("datapath:")] == ["datapath:0"]       # the f32 filter sees its own only
    assert [ln for ln in log if ln.startswith("datapath_i8:")] == ["datapath_i8:0"]
    assert not any("datapath_f16" in ln for ln in log0)


@pytest.mark.parametrize("mode,want", [("stuck_bit", "stage 4 word 0 xor 0x40000000 (bit 30)"),
                                       ("missing", "254/256 workgroups exact"), ("device_bad", "device_bad=12")])
def test_stub_fault_modes_in_serve_and_one_shot(tmp_path, mode, want):
    control = {"datapath_f16": {"3": mode}}
    (reply_hello, bad, good, f32), _ = _serve(tmp_path, mode, ["datapath_f16 5 3:1", "datapath_f16 5 2:2",
                                                                "datapath 5 3:3"], control)
    assert bad["ok"] is False and bad["devices"][0]["ok"] is False and want in bad["devices"][0]["error"]
    assert good["ok"] is True and f32["ok"] is True       # another device, and the f32 check of the same device
    ctl = tmp_path / "one.json"
    ctl.write_text(json.dumps(control))
    for ordinal, rc in (("3", 1), ("2", 0)):
        p = subprocess.run([sys.executable, STUB, "--devices", "0", "--nonce", "77", "--datapath-f16"],
                           capture_output=True, text=True, timeout=20,
                           env=dict(os.environ, MI355X_STUB_PROBE_CONTROL=str(ctl), ROCR_VISIBLE_DEVICES=ordinal))
        doc = json.loads(p.stdout)
        assert p.returncode == rc and doc["datapath_f16"] is True and "datapath" not in doc
        assert doc["devices"][0]["nonce"] == 77 and (want in doc["devices"][0]["error"]) == (rc == 1)
