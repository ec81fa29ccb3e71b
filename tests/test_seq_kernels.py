"""The recurrent kernels (csrc/kernels_seq.h, csrc/kernels_seq_stream.h) at every template instance the launch plans of
csrc/seq_launch.h can hand a layer, each pinned by one single-layer case against a float64 reference (tests/seq_kernel_suite.py).

Which kernel takes a recurrence is invisible to every parity test -- all of them compute the same numbers -- and decides the speed of
the benchmarked step.  tests/golden/seq_plans_v1.json pins the selection: for a fixed list of calls on both sides of every rule edge
(supported and unsupported widths and hop counts; 1, 15, 16, 20, 21, 32 nodes; clip counts around 256, 384 and 512; spectral or not;
every tensor size the rules compare with the 2 GB a descriptor reaches, one step below and at it; each dev knob alone; the probe flag
with and without -DEEG_DEV) the plan the code gave when the file was recorded.  A change of selection shows up here; where it is
wanted, the file is rewritten (`python tests/seq_kernel_suite.py --record tests/golden/seq_plans_v1.json`) and the commit says why.
A recording pins changes, not correctness, so the recorded plans are also held against what does not come from the code under test:
the LDS of a CU, the grids, the block of the two-wave kinds, the existence predicates, and eeg_dcrnn_supported.

Without a GPU the case table must plan exactly the instances the rules can reach: 16 / 32 / 64 units x M in {1, 2, 3, 4, 5, 7} x
1 .. 32 nodes x clip counts around 256 / 384 / 512 x spectral or not, and one layer past 2 GB.  ONE exclusion: the one-wave kernels at
64 units, M <= 3, N <= 20 (seq_fwd_kernel / seq_bwd_kernel<64, 1|2|3, 5, false>) are planned by a product build only where a tensor
of the call is beyond the 2 GB a buffer descriptor reaches, which no test allocates; they run on the emulator under the one-wave dev
knobs with the same checks (tests/test_emu_parity.py).  The forward instance at 64 units, M = 7 above 20 nodes is planned but never
launched: the backward of that shape does not fit the LDS and the layer is refused as a whole, so the enumeration counts layers, not
plans.  With a GPU (`-m gpu`): every case proves through the event recorder that the kernels it names took `seq_fwd` and `seq_bwd`,
then compares hidden sequence and all gradients, and repeats the forward without saving for a backward (bit-equal); the walk cases
(one clip more than the grid) run again with a cotangent on four clips only."""
import json
import os
import re

import pytest
import torch

import quad_gemm_suite as qg
import seq_kernel_suite as sk

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


@pytest.fixture(scope="module")
def plan_driver_product(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver_product"), dev=False)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "seq_plans_v1.json")) as f:
        return json.load(f)


@pytest.fixture
def hip_library():
    from eeg_gnn_ssl_amd import _lib
    _lib._LIB = None
    lib = _lib.get_lib()                  # ImportError if the HIP library is missing: no fallback
    assert lib.is_device_build and os.path.basename(lib.path) == "libeeg_dcrnn_hip.so"
    assert torch.cuda.is_available()
    torch.set_num_threads(16)             # (the float64 reference: a fraction of a second per case)
    yield lib


def _fields(call):
    f = call.split()
    keys = ("H", "M", "N", "T", "B", "plane_stride", "spectral", "Sp", "SpE", "one_wave", "no_spec", "stream", "probe")
    return dict(zip(keys, (int(v) for v in f[1:])), dir=f[0][1:])


# ---- no GPU: the recorded selection ---------------------------------------------------------------------------------------------
def test_seq_launch_plans_match_the_recorded_selection(plan_driver, plan_driver_product, recorded):
    for key, exe, least in (("plans", plan_driver, 300), ("plans_product", plan_driver_product, 30)):
        plans = recorded[key]
        assert len(plans) >= least
        out = sk.drive(exe, [p["call"] for p in plans])
        wrong = [(p["call"], p["plan"], got) for p, got in zip(plans, out) if got != p["plan"]]
        assert not wrong, "%s: %d of %d plans changed; first (call, recorded, now): %s" % (key, len(wrong), len(plans), wrong[:3])
    # a call without the probe flag is planned alike by both builds: the product build against the whole recording
    plain = [p for p in recorded["plans"] if not _fields(p["call"])["probe"]]
    out = sk.drive(plan_driver_product, [p["call"] for p in plain])
    wrong = [(p["call"], p["plan"], got) for p, got in zip(plain, out) if got != p["plan"]]
    assert len(plain) >= 250 and not wrong, "product build: %d of %d plans changed; first (call, recorded, now): %s" % (len(wrong), len(plain), wrong[:3])


def test_recorded_calls_sit_on_both_sides_of_every_rule_edge(recorded):
    calls = [_fields(p["call"]) for p in recorded["plans"]]
    plans = [sk.parse_plan(p["plan"]) for p in recorded["plans"]]
    assert [p["call"] for p in recorded["plans"]] == sk.recorded_calls()[0] and [p["call"] for p in recorded["plans_product"]] == sk.recorded_calls()[1]
    for key, must in (("H", {8, 16, 32, 48, 64}), ("M", set(range(9))), ("N", {1, 15, 16, 20, 21, 32}), ("B", {1, 255, 256, 257, 383, 384, 511, 512, 513}),
                      ("spectral", {0, 1}), ("one_wave", {0, 1}), ("no_spec", {0, 1}), ("stream", {0, 1, 2}), ("probe", {0, 1})):
        assert must <= {c[key] for c in calls}, key
    for direction in ("fwd", "bwd"):
        mine = [c for c in calls if c["dir"] == direction]
        sizes = {"T*B*N*H": lambda c: c["T"] * c["B"] * c["N"] * c["H"], "T*B*N*3H": lambda c: c["T"] * c["B"] * c["N"] * 3 * c["H"],
                 "N*Sp*3H": lambda c: c["N"] * c["Sp"] * 3 * c["H"], "N*SpE*H": lambda c: c["N"] * c["SpE"] * c["H"],
                 "(M-1)*plane_stride": lambda c: (c["M"] - 1) * c["plane_stride"]}
        for what, size in sizes.items():
            step = 3 * 16 * 64 if "3H" in what else 16 * 64 if what != "(M-1)*plane_stride" else 4          # (the call list's granule: 16 nodes, 64 units)
            seen = {size(c) for c in mine}
            assert any(sk.REACH - step <= v < sk.REACH for v in seen) and any(sk.REACH <= v < sk.REACH + step for v in seen), (direction, what)
    kinds = {(c["dir"], p["kind"], p["probe"]) for c, p in zip(calls, plans) if not p["error"]}
    assert kinds == {(d, k, pr) for d in ("fwd", "bwd") for k in sk.KINDS[:3] for pr in (False, True)} | {("bwd", "stream", False)}
    assert {p["error"] for p in plans} == {0, 1, 2}
    assert not any(sk.parse_plan(p["plan"])["probe"] for p in recorded["plans_product"])        # no probe instantiation in a product build


def test_recorded_plans_respect_what_the_device_and_the_kernels_fix(plan_driver, plan_driver_product, recorded):
    """of every recorded plan without an error: the LDS of a CU, the grid (one workgroup per clip up to one per CU, two for the streamed
    kernel), the block of the two-wave kinds, and a kind only where the existence predicate of kernels_seq.h holds"""
    for key, exe, dev in (("plans", plan_driver, 1), ("plans_product", plan_driver_product, 0)):
        calls = [_fields(p["call"]) for p in recorded[key]]
        plans = [sk.parse_plan(p["plan"]) for p in recorded[key]]
        shapes = sorted({(c["H"], c["M"], c["N"]) for c in calls})
        has = {s: [int(v) for v in ln.split()] for s, ln in zip(shapes, sk.drive(exe, ["shas %d %d %d" % s for s in shapes]))}
        for c, p in zip(calls, plans):
            nks, two_wave, spec, probe, stream, h_ok, m_ok, dev_build = has[(c["H"], c["M"], c["N"])]
            assert dev_build == dev and nks == (5 if c["N"] <= 20 else 8)
            if p["error"]:
                assert p["error"] == 2 or not (h_ok and m_ok), (c, p)
                continue
            assert h_ok and m_ok and 0 < p["lds"] <= sk.LDS_BYTES and p["nks"] == nks, (c, p)
            assert p["grid"] == min(c["B"], sk.STREAM_GRID if p["kind"] == "stream" else sk.SEQ_GRID), (c, p)
            assert p["block"] == (512 if p["kind"] in ("two_wave", "two_wave_spec") else 256), (c, p)
            assert p["kind"] != "two_wave" or two_wave, (c, p)
            assert p["kind"] != "two_wave_spec" or (spec and c["spectral"] and 16 <= c["N"] <= 20), (c, p)
            assert p["kind"] != "stream" or (stream and c["dir"] == "bwd" and c["N"] <= 20 and 2 * p["lds"] <= sk.LDS_BYTES), (c, p)
            assert not p["probe"] or (probe and c["probe"]), (c, p)


def test_supported_shapes_are_the_ones_both_plans_accept(plan_driver):
    """eeg_dcrnn_supported (the emulator build of api.cpp) refuses exactly the (N, H, M) for which the forward or the backward plan of a
    layer reports an error"""
    import emu_support
    shapes = [(n, h, m) for n in range(1, 33) for h in (8, 16, 32, 48, 64, 128) for m in range(0, 9)]
    out = sk.drive(plan_driver, [ln for n, h, m in shapes for ln in sk.layer_calls(h, m, n, 2, 3)])
    planned_ok = [not sk.parse_plan(out[2 * i])["error"] and not sk.parse_plan(out[2 * i + 1])["error"] for i in range(len(shapes))]
    lib = emu_support.install_emulator()
    try:
        supported = [bool(lib.query("eeg_dcrnn_supported", n, h, 4, m)) for n, h, m in shapes]
    finally:
        emu_support.uninstall()
    wrong = [(s, a, b) for s, a, b in zip(shapes, supported, planned_ok) if a != b]
    assert not wrong, "(N, H, M), supported, planned without error: %s" % wrong[:5]
    assert sum(supported) == 3 * 6 * 32 - 12          # 64 units with 7 hop matrices above 20 nodes: the BPTT tiles exceed the LDS


# ---- no GPU: the table against the selection rules -------------------------------------------------------------------------------
def test_case_table_plans_what_it_names(plan_driver, plan_driver_product):
    """each case is planned by seq_launch.h -- development and product build alike -- as the kernels its `expect` names; the cases
    under dev knobs as theirs"""
    for exe in (plan_driver, plan_driver_product):
        for (name, case), roles in zip(sk.CASES.items(), sk.planned(exe, [sk.case_layer(c) for c in sk.CASES.values()])):
            assert roles == case["expect"], (name, roles)
    knobbed = sk.planned(plan_driver, [sk.case_layer(sk.CASES[base], knobs) for base, knobs, _ in sk.KNOB_CASES.values()])
    for (name, (base, knobs, expect)), roles in zip(sk.KNOB_CASES.items(), knobbed):
        assert roles == expect and roles != sk.CASES[base]["expect"] and sk.CASES[base]["b"] <= 5, (name, roles)
    # the instances out of a product build's reach run on the emulator; so does a small case of every template and every H
    assert set(sk.EXCLUDED) <= {s for _, _, expect in sk.KNOB_CASES.values() for s in expect.values()}
    assert {sk.stream(m) for m in (1, 2, 3)} <= {expect["seq_bwd"] for _, _, expect in sk.KNOB_CASES.values()}
    emu = [sk.CASES[name] for name in sk.EMU_CASES]
    assert all(c["b"] <= 5 for c in emu) and {c["h"] for c in emu} == set(sk.HS)
    emu_templates = {sk.template_of(s) for c in emu for s in c["expect"].values()} | {sk.template_of(s) for _, _, e in sk.KNOB_CASES.values() for s in e.values()}
    assert emu_templates == {sk.template_of(s) for c in sk.CASES.values() for s in c["expect"].values()}
    assert any(c["h"] == 64 and qg.hops(c) == 7 for c in emu)            # the 20-row backward layout


def test_case_table_covers_every_reachable_recurrent_instance(plan_driver_product):
    """16 / 32 / 64 units x every supported hop count x 1 .. 32 nodes x clip counts around 256 / 384 / 512 x spectral or not, no dev
    knobs, and one layer past the 2 GB reach per shape: the kernel instances those layers are planned with are exactly the ones the
    case table names, plus the exclusion -- a rule change that reaches another instance fails here until a case runs it"""
    below, beyond = sk.reachable_instances(plan_driver_product)
    named = {s for case in sk.CASES.values() for s in case["expect"].values()}
    excluded = set(sk.EXCLUDED)
    assert all(re.fullmatch(r"seq_(fwd|bwd)_kernel<64, [123], 5, false>", s) for s in excluded) and all(sk.EXCLUDED.values())
    assert not excluded & below and not excluded & named, "an excluded instance is within a product build's reach below 2 GB: it needs a case"
    assert below == named, {"reachable without a case": sorted(below - named), "named but unreachable": sorted(named - below)}
    assert below | beyond == named | excluded, {"reachable, neither named nor excluded": sorted((below | beyond) - named - excluded),
                                               "excluded but unreachable": sorted(excluded - beyond)}
    fwd = {s for s in below if s.startswith("seq_fwd")}
    # forward: 32 one-wave instances (36 less the three two-wave shapes and 64 units x M = 7 above 20 nodes, whose backward is refused), three
    # two-wave, two SPEC; backward: the same 32 + 3 + 2 and the two streamed instances a product build plans (M = 4, 5)
    assert (len(fwd), len(below - fwd), len(excluded)) == (37, 39, 6)
    assert len(below | beyond) == 82


def test_case_table_holds_the_edges_it_is_there_for():
    cases = sk.CASES.values()
    assert {1, 2, 15, 16, 17, 19, 20, 21, 31, 32} <= {c["n"] for c in cases}
    assert 1 in {c["t"] for c in cases} and max(c["t"] for c in cases) >= 3 and all(c["t"] <= 3 for c in cases)
    assert {c["act"] for c in cases} == {"tanh", "relu"}
    assert 3 * sum(c["h0"] for c in cases) >= len(sk.CASES) and {c["h"] for c in cases if c["h0"]} == set(sk.HS)
    assert all(4 <= c["fin"] <= 20 or c["spectral"] for c in cases)       # (the input gradient of a spectral layer needs Fin = 64)
    assert all(2 <= c["b"] <= 5 or c["b"] in (383, 384) or name in sk.WALK_CASES for name, c in sk.CASES.items())
    # ragged lengths hold a clip of length 1 and one of length T
    ragged = [name for name, c in sk.CASES.items() if c["lengths"]]
    assert len(ragged) >= 8 and {sk.CASES[name]["h"] for name in ragged} == set(sk.HS)
    for name in ragged:
        case = sk.CASES[name]
        lengths = qg.make_operands(case, case["t"], case["b"], 0)["lengths"].tolist()
        assert case["t"] >= 2 and 1 in lengths and case["t"] in lengths, (name, lengths)
    # one shared graph (p_batched = 0) that is not symmetric: the general path; per-clip graphs; the spectral form
    assert any(c["p_batched"] == 0 and not c["spectral"] for c in cases) and any(c["p_batched"] == 1 for c in cases)
    sup = qg.make_supports(sk.CASES["h16_m2_n15"], 3, torch.Generator().manual_seed(0))
    assert len(sup) == 1 and sup[0].dim() == 2 and not torch.equal(sup[0], sup[0].t())
    sym = qg.make_supports(sk.CASES["h64_m2_n16_spec"], 3, torch.Generator().manual_seed(0))
    assert len(sym) == 1 and sym[0].dim() == 2 and torch.allclose(sym[0], sym[0].t(), atol=1e-6)
    # a spectral request below 16 nodes falls to the plain two-wave kernels
    assert any(c["spectral"] and c["n"] < 16 and c["expect"] == {"seq_fwd": sk.fwd2(qg.hops(c)), "seq_bwd": sk.bwd2(qg.hops(c))} for c in cases)
    # the two sides of the streamed rule
    sides = {c["b"]: c for c in cases if c["b"] in (383, 384) and qg.hops(c) in (4, 5)}
    assert sides[383]["expect"]["seq_bwd"] == sk.bwd1(64, qg.hops(sides[383]), 5) and sides[384]["expect"]["seq_bwd"] == sk.stream(qg.hops(sides[384]))
    assert {k: v for k, v in sides[383].items() if k not in ("b", "expect")} == {k: v for k, v in sides[384].items() if k not in ("b", "expect")}


def test_walk_cases_hand_exactly_one_workgroup_a_second_clip():
    walks = [sk.CASES[name] for name in sk.WALK_CASES]
    for case in walks:
        assert case["b"] == sk.grid_of(case) + 1 and case["t"] <= 2, case
    assert [c["b"] for c in walks if c["expect"]["seq_bwd"].startswith("seq_bwd_stream_kernel")] == [513]
    templates = {sk.template_of(s) for c in walks for s in c["expect"].values()}
    assert templates == {"seq_fwd_kernel NKS=5", "seq_fwd_kernel NKS=8", "seq_bwd_kernel NKS=5", "seq_bwd_kernel NKS=8", "seq_fwd2_kernel SPEC=false",
                         "seq_fwd2_kernel SPEC=true", "seq_bwd2_kernel SPEC=false", "seq_bwd2_kernel SPEC=true", "seq_bwd_stream_kernel"}
    assert any(c["h"] == 64 and qg.hops(c) == 7 and c["n"] <= 20 for c in walks)                  # the 20-row backward layout
    assert {c["h"] for c in walks} == set(sk.HS)
    assert sk.sparse_clips(257, 256) == [0, 255, 256] and sk.sparse_clips(513, 512) == [0, 511, 512]


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sk.CASES))
def test_seq_kernel_case(hip_library, name):
    sk.check_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sk.WALK_CASES))
def test_seq_kernel_walk_case_sparse_cotangent(hip_library, name):
    sk.check_case(name, "cuda", sparse=True)
