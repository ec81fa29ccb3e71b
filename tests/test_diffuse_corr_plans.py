"""Which kernel takes a hop-diffusion call (csrc/diffuse_launch.h) or a correlation-Gram call (csrc/corr_launch.h) is invisible to every
parity test -- the streaming and the LDS diffusion give the same numbers, and so do all the Gram instances -- but it decides cfg2 / cfg5
time.  tests/golden/diffuse_plans_v1.json and corr_plans_v1.json pin it: for short lists of calls that straddle every rule (diffusion:
node counts 19 / 20 / 32 / 5, row widths on both sides of F/4 <= 128, 1 / 3 / 4 / 5 samples per graph, shared and per-clip graphs, every hop count, T and F
across each halving of the workgroup, grids on both sides of their clamps, the adjoint's 32-bit-offset bound, column chunks by the LDS
bound and by the forward's prefetch bound, the batch-major input, each dev knob; Gram: every width 4 .. 132, node counts on both sides
of 20 and of 32, with and without lengths, B and T on both sides of the split's cap and target, raw rows and window tensors on both
sides of a chunk, the 65535 clamp, every refusal) what the selection code gave before it was gathered into those headers.  A change of
selection shows up here; where it is wanted, the files are rewritten from the driver's own output (same call lines) and the commit
says why.

The restated rules of tests/diffuse_corr_suite.py are held against the driver over whole grids, the reachable instances are exactly
the compiled ones, and the workspace entry points of the library answer as the plans.  tests/test_diffuse_corr_kernels.py ties the
plans to what runs."""
import itertools
import json
import os
import subprocess

import pytest

import diffuse_corr_suite as dc
import quad_gemm_suite as qg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "eeg_gnn_ssl_amd", "csrc")


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


def _drive(exe, calls):
    out = subprocess.run([exe], input="".join(c + "\n" for c in calls), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(calls)
    return out


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)["plans"]


@pytest.mark.parametrize("name, least", [("diffuse_plans_v1.json", 400), ("corr_plans_v1.json", 450)])
def test_launch_plans_match_the_recorded_selection(plan_driver, name, least):
    plans = _golden(name)
    assert len(plans) >= least
    out = _drive(plan_driver, [p["call"] for p in plans])
    wrong = [(p["call"], p["plan"], got) for p, got in zip(plans, out) if got != p["plan"]]
    assert not wrong, "%d of %d plans changed; first (call, recorded, now): %s" % (len(wrong), len(plans), wrong[:3])


def test_goldens_hold_every_instance_and_every_refusal():
    d = [p["plan"] for p in _golden("diffuse_plans_v1.json")]
    c = _golden("corr_plans_v1.json")
    seen = {dc.symbol_of(p) for p in d if " ; " in p} | {f for p in c for f in p["plan"].split(" ; ")[0:3:2] if " ; " in p["plan"]}
    assert seen == dc.COMPILED
    assert {p for p in d if " ; " not in p} == {"none", "error 1", "error 2"}
    for op, codes in (("gram", 5), ("grows", 7)):
        assert {p["plan"] for p in c if p["call"].startswith(op + " ") and p["plan"].startswith("error")} == {f"error {k}" for k in range(1, codes + 1)}
    chunks = {p.split(" ; ")[2].split()[0] for p in d if " ; x" in p}
    assert {"x1", "x2", "x4", "x8"} <= chunks                     # Fc == F, chunked once, twice, three times


@pytest.mark.parametrize("header, probe", [("diffuse_launch.h", "eeg::diffuse_plan(eeg::DiffuseCall{0, 8, 2, 19, 8, 3, false}).kind == eeg::DiffuseKind::StreamFwd"),
                                           ("corr_launch.h", "eeg::corr_gram_plan(2, 6, 19, 100, false, 0).nq == 7")],
                         ids=["diffuse_launch.h", "corr_launch.h"])
def test_launch_header_is_host_code_on_its_own(tmp_path, header, probe):
    """the header alone, with the driver's compiler and flags: no kernel bodies, nothing but common.h"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return %s ? 0 : 1; }\n' % (header, probe))
    subprocess.check_call([qg.CLANG if os.path.exists(qg.CLANG) else "clang++", "-x", "c++", "-std=c++17", "-O1", "-DEEG_PLATFORM_HEADER=\"platform_emu.h\"",
                           "-DEEG_DEV", "-I", os.path.join(HERE, "emu"), "-I", CSRC, "-Wno-unused-function", "-Wno-unknown-attributes", "-fsyntax-only", str(src)])
    with open(os.path.join(CSRC, header)) as f:
        text = f.read()
    assert "__global__" not in text
    assert [ln.split('"')[1] for ln in text.splitlines() if ln.startswith("#include")] == ["common.h"]


# ---- the restated rules against the driver, over whole grids ---------------------------------------------------------------------------
DIFFUSE_KNOBS = ((0, 0, 0, 0), (16, 0, 0, 0), (0, 16, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (300, 5000, 1, 1))


def _diffuse_grid():
    for adjoint, pb, n, f, m, spg, b, kn in itertools.product((0, 1), (0, 1), (1, 5, 18, 19, 20, 21, 32), (4, 8, 12, 36, 64, 100, 128, 132, 200, 508, 512, 516, 1000),
                                                              range(1, 9), (1, 2, 3, 4, 5, 7, 31, 33, 300), (1, 3, 700), DIFFUSE_KNOBS):
        yield (adjoint, pb, spg * b, b, n, f, m, 0, 0) + kn
    for pb, n, f, m, spg, x_bt, copy in itertools.product((0, 1), (19, 20), (8, 512, 516), (1, 2), (3, 4), (0, 1, 2), (0, 1)):
        yield (0, pb, spg * 2, 2, n, f, m, x_bt, copy, 0, 0, 0, 0)
    for adjoint, s, m in itertools.product((0, 1), (249647, 249648, 3000000), (1, 7)):          # the adjoint's S*N*M*F < 1.7e10
        yield (adjoint, 0, s, 1, 19, 512, m, 0, 0, 0, 0, 0, 0)


def test_diffusion_rules_restated_answer_as_the_plan_over_the_whole_grid(plan_driver):
    grid = list(_diffuse_grid())
    assert len(grid) > 200000
    out = _drive(plan_driver, [("dadj " if g[0] else "dfwd ") + " ".join(map(str, g[1:])) for g in grid])
    restated = [dc.diffuse_line(*g) for g in grid]
    wrong = [(g, line, want) for g, line, want in zip(grid, out, restated) if line != want]
    assert not wrong, "%d differ; first (call, plan, restated): %s" % (len(wrong), wrong[:3])
    reach = lambda rows: {dc.symbol_of(line) for g, line in rows if " ; " in line}          # noqa: E731
    diffusion = {s for s in dc.COMPILED if s.startswith("diffuse")}
    assert reach(zip(grid, out)) == diffusion and len(diffusion) == 6
    assert reach((g, line) for g, line in zip(grid, out) if g[9:] == (0, 0, 0, 0)) == diffusion - dc.KNOB_ONLY
    # fewer than 4 samples per graph (a decoder step) never stream; the montage with 4 or more does, in both directions
    for g, line in zip(grid, out):
        if " ; " in line and g[9:] == (0, 0, 0, 0):
            per_graph = g[2] // (g[3] if g[1] else 1)
            streams = dc.symbol_of(line) not in (dc.FWD_LDS, dc.ADJ_LDS)
            offsets_fit = not g[0] or g[2] * g[4] * g[6] * g[5] < 1.7e10
            assert streams == (g[4] == 19 and g[5] <= 512 and per_graph >= 4 and offsets_fit), (g, line)
    assert dc.diffuse_line(1, 1, 8, 2, 19, 8, 5).startswith(dc.adj_rows(5)) and dc.diffuse_line(1, 1, 6, 2, 19, 8, 5).startswith(dc.ADJ_LDS)


def _gram_grid():
    for b, t, n, d, ln, kn in itertools.product((0, 1, 2, 7, 256, 1023, 1024, 1025, 5000), (0, 1, 3, 4, 5, 8, 9, 100, 585, 586, 4095, 4096, 4097, 4100, 9000),
                                                (0, 1, 16, 19, 20, 21, 31, 32, 33), tuple(range(0, 141, 4)) + (6, 10, 130), (0, 1), (0, 1, 100, 100000)):
        yield b, t, n, d, ln, kn


def _rows_grid():
    for b, n, (p, q), ln, kn in itertools.product((0, 1, 2, 300, 1024, 1025), (0, 1, 19, 20, 21, 32, 33),
                                                  ((0, 8), (1, 0), (1, 4), (1, 6), (1, 252), (1, 256), (1, 260), (1, 520), (1, 1024), (1, 1028), (1, 12000), (1, 1 << 20),
                                                   (1, 1 << 24), (1, (1 << 24) - 4), (3, 8), (12, 200), (60, 256), (60, 260), (4100, 4)), (0, 1), (0, 1, 100, 1 << 20)):
        for ps, steps in itertools.product((0, n * q - 4, n * q, n * q + 2, n * q + 4, 1 << 27), (0, 1, 3, 5, p)):
            if ln or steps == 0:
                yield b, n, p, q, ps, ln, steps, kn
    for q in (4 * 65534 * 256, 4 * 65535 * 256, 4 * 65535 * 256 + 4, 4 * 65536 * 256):          # the 65535 clamp of grid.y
        for kn in (0, 65535, 65536, 1 << 20):
            yield 1, 1, 1, q, 0, 0, 0, kn


def test_gram_rules_restated_answer_as_the_plan_over_the_whole_grid(plan_driver):
    gram, rows = list(_gram_grid()), list(_rows_grid())
    assert len(gram) > 100000 and len(rows) > 100000
    out = _drive(plan_driver, ["gram " + " ".join(map(str, g)) for g in gram])
    wrong = [(g, line, want) for g, line, want in zip(gram, out, (dc.gram_line(*g) for g in gram)) if line != want]
    assert not wrong, "%d differ; first (call, plan, restated): %s" % (len(wrong), wrong[:3])
    out_r = _drive(plan_driver, ["grows " + " ".join(map(str, g)) for g in rows])
    wrong = [(g, line, want) for g, line, want in zip(rows, out_r, (dc.rows_line(*g) for g in rows)) if line != want]
    assert not wrong, "%d differ; first (call, plan, restated): %s" % (len(wrong), wrong[:3])

    def reach(pairs):
        return {s for g, line in pairs if " ; " in line for s in line.split(" ; ")[0:3:2]}
    corr = {s for s in dc.COMPILED if s.startswith("corr")}
    assert reach(zip(gram, out)) | reach(zip(rows, out_r)) == corr and len(corr) == 37
    assert reach((g, ln) for g, ln in zip(gram, out) if g[-1] == 0) | reach((g, ln) for g, ln in zip(rows, out_r) if g[-1] == 0) == corr - dc.KNOB_ONLY


def test_every_compiled_instance_is_reachable_and_none_needs_a_knob():
    """43 instances in all, none of them reachable under a dev knob only: the product library runs every case of the suite, and the
    development-build parametrisation has nothing to add (at most len(KNOB_ONLY) = 0 cases)"""
    assert len(dc.COMPILED) == 43 and len(dc.KNOB_ONLY) == 0
    named = {c["expect"] for c in dc.DIFFUSE_CASES.values()} | {c["expect"] for c in dc.CORR_CASES.values()} | {dc.FINISH}
    assert named == dc.COMPILED, {"compiled without a case": sorted(dc.COMPILED - named), "named but not compiled": sorted(named - dc.COMPILED)}


def test_case_table_is_planned_as_it_names(plan_driver):
    cases = list(dc.DIFFUSE_CASES.items()) + list(dc.CORR_CASES.items())
    lines = [dc.case_line(c) for _, c in cases]
    out = _drive(plan_driver, [call for call, _ in lines])
    for (name, c), (call, restated), line in zip(cases, lines, out):
        assert line == restated and dc.symbol_of(line) == c["expect"], (name, call, line, restated)
        if "adjoint" in c and " ; x" in line:
            assert int(line.split(" ; x")[1].split()[0]) == c["launches"], (name, line)
    # the case table holds the edges it is there for: a ragged column chunk, a ragged split, a ragged row chunk
    assert dc.diffuse_line(0, 1, 4, 2, 32, 132, 3).endswith("x2 80") and dc.diffuse_line(1, 1, 4, 2, 32, 132, 3).endswith("x1 132")
    assert dc.gram_line(1, 9, 19, 100, 0).split(" ; ")[1] == "1 3 256 32768"
    assert dc.rows_line(2, 19, 1, 520, 0, 0, 0).split(" ; ")[1].split()[1] == "1" and 520 % dc.ROW_CHUNK != 0


# ---- the workspace entry points answer as the plans -------------------------------------------------------------------------------------
def test_workspace_entry_points_agree_with_the_plans():
    import emu_support
    lib = emu_support.install_emulator()
    try:
        checked = 0
        for p in _golden("corr_plans_v1.json"):
            if p["plan"].startswith("error"):
                continue
            op, *f = p["call"].split()
            f = [int(v) for v in f]
            lib.call("eeg_dcrnn_set_tuning", 7, f[-1])
            got = lib.query("eeg_dcrnn_corr_graph_ws_floats", f[0], f[1]) if op == "gram" else lib.query("eeg_dcrnn_corr_graph_rows_ws_floats", f[0], f[2], f[3])
            assert got == int(p["plan"].split(" ; ")[-1]), (p, got)
            checked += 1
        assert checked > 350
    finally:
        lib.call("eeg_dcrnn_set_tuning", 7, 0)
        emu_support.uninstall()
