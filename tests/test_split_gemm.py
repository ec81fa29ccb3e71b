"""The split GEMMs (csrc/kernels_gemm.h; the opt-in gemm_nn_bf3_kernel of kernels_gemm_bf.h) at every template instance a product
build can reach, each pinned on the MI355X by a dconv call or a single layer against a float64 reference (tests/split_gemm_suite.py).

Without a GPU: the plan driver enumerates the instances that the selection rules of csrc/gemm_launch.h hand to layers, dconv calls
and the decoder's projection from 19 to 291 840 rows, and the case tables must name exactly that set -- a rule change that makes
another instance reachable fails here until a case runs it; the edges the table is there for (partial tiles and column blocks, empty
and short row splits, straddling k-blocks) are asserted from the driver's lines.  With one (`-m gpu`): every case proves through the
event recorder that the kernels it names took its GEMMs, then compares outputs and gradients; three dconv cases run again with a
cotangent on a few clips only.  The emulator twins, and the instances only dev knobs reach, are in tests/test_emu_parity.py."""
import os

import pytest
import torch

import quad_gemm_suite as qg
import split_gemm_suite as sg

TABLE_CUS = sg.TABLE_CUS


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


@pytest.fixture
def hip_library():
    from eeg_gnn_ssl_amd import _lib
    _lib._LIB = None
    lib = _lib.get_lib()                  # ImportError if the HIP library is missing: no fallback
    assert lib.is_device_build and os.path.basename(lib.path) == "libeeg_dcrnn_hip.so"
    assert torch.cuda.is_available()
    torch.set_num_threads(16)             # (the float64 reference: about a second per case)
    yield lib


# ---- no GPU: the tables against the selection rules ----------------------------------------------------------------------------------
def test_case_table_plans_what_it_names(plan_driver):
    """each case, at 256 CUs, is planned by gemm_launch.h as the kernels its `expect` names; and the edges the dconv table is there for,
    read from the driver's lines"""
    cases = list(sg.DCONV_CASES.items())
    plans = sg.dconv_planned(plan_driver, [c["dims"] for _, c in cases], cus=TABLE_CUS)
    facts = {}
    for (name, case), (symbols, fact) in zip(cases, plans):
        assert symbols == case["expect"], (name, symbols)
        assert fact["remap"] == case["tn"]["remap"], (name, fact)
        empty = fact["nsplit"] - -(-fact["r"] // fact["rps"])
        assert empty == case["tn"].get("empty", 0), (name, fact)
        m, f, n, b, o, pb = case["dims"]
        facts[name] = dict(fact, m=m, f=f, o=o, pb=pb, empty=empty, tn=symbols["tn"])
        assert f in (4, 16, 20, 36, 68, 100) and m <= 7 and o % 16 == 0 and o <= 192, name
    fs = list(facts.values())
    # every reachable instance is named (test_case_table_covers_every_reachable_split_instance: and no other)
    assert len(sg.named_instances()) == 13
    assert {s for c in sg.DCONV_CASES.values() for s in c["expect"].values()} == sg.named_instances()      # dconv alone reaches them all
    # each DMA TN instance with and without the XCD placement
    for sym in (sg.tn_dma(2, 32), sg.tn_dma(4, 32), sg.tn_dma(6, 16)):
        assert {x["remap"] for x in fs if x["tn"] == sym} == {0, 1}, sym
    # NN: a partial last column block at NCTW = 4 and at NCTW = 6 (forward or input gradient)
    nn = [(x, x[g + "_nctw"], x[g + "_nct"], x[g + "_gy"]) for x in fs for g in ("fwd", "dx")]
    for nctw in (4, 6):
        assert any(w == nctw and nct % (2 * nctw) != 0 and gy == -(-nct // (2 * nctw)) for _, w, nct, gy in nn), nctw
    assert any(w == 2 and gy >= 3 and nct % 4 != 0 for _, w, nct, gy in nn)
    assert any((x["m"] * x["f"]) % 16 != 0 for x in fs)                                   # the last column tile of dX is wider than ldc = O = M*F
    assert facts["r57_m3_f20"]["m"] * facts["r57_m3_f20"]["f"] == 60
    assert any(x["m"] == 7 for x in fs) and any(x["m"] == 1 for x in fs)                  # seven segments in one launch; none to diffuse
    assert any(x["r"] < 128 for x in fs)
    assert any(x["r"] % 128 != 0 and w >= 4 for x, w, _, _ in nn)                         # a partial last row tile under wide column blocks
    assert {w for _, w, _, _ in nn} == {2, 4, 5, 6}
    assert any(x["dx_nct"] > 12 and x["dx_nct"] <= 24 and x["r"] < 20353 and x["dx_nctw"] == 6 for x in fs)   # 13..24 tiles: wide blocks from 10 113 rows
    # TN: empty trailing splits, R % 32 != 0 under 32-row stages, a short last split, a k-block across two segments, a ragged K
    dma = [x for x in fs if x["tn"] != sg.tn_staged(1)]
    assert any(x["empty"] > 0 and x["remap"] == 1 for x in dma)
    assert any(x["r"] % 32 != 0 for x in dma) and any(x["r"] % 32 != 0 for x in fs if x["tn"] == sg.tn_staged(1))
    assert any(x["r"] % x["rps"] != 0 and x["nsplit"] > 1 for x in dma)
    assert any(x["f"] % 64 != 0 and x["m"] >= 2 for x in dma)
    assert any((x["m"] * x["f"]) % 64 != 0 for x in dma)
    assert any(x["rps"] > 128 for x in fs)
    assert {x["o"] for x in fs} >= {16, 32, 48, 80, 144, 176, 192}
    assert {x["pb"] for x in fs} == {0, 1} and {x["pb"] for x in fs if x["r"] > 20352} == {0, 1}
    # the sparse reruns: one per width of the DMA TN kernel, one with empty trailing splits, at least three distinct clips each
    assert {facts[n]["tn"] for n in sg.DCONV_SPARSE_CASES} == {sg.tn_dma(2, 32), sg.tn_dma(4, 32), sg.tn_dma(6, 16)}
    assert any(facts[n]["empty"] > 0 for n in sg.DCONV_SPARSE_CASES)
    clips = [sg.dconv_sparse_clips(sg.DCONV_CASES[n]["dims"][3], sg.DCONV_CASES[n]["dims"][2], facts[n]["rps"]) for n in sg.DCONV_SPARSE_CASES]
    assert sorted(len(c) for c in clips) == [3, 4, 4], clips                              # (w4_f100: its last split starts inside the last clip)


def test_layer_and_bf16_split_cases_plan_what_they_name(plan_driver):
    t, b, r = sg.LAYER_DIMS
    assert r == t * b * 19 and 20352 < r < 256 * TABLE_CUS and b < 384 and r % 128 == 16
    layers = [(c["h"], qg.hops(c), c["fin"], r, c["bm"], TABLE_CUS) for c in sg.LAYER_CASES.values()]
    for (name, case), (roles, _) in zip(sg.LAYER_CASES.items(), qg.planned(plan_driver, layers)):
        assert roles == case["expect"], (name, roles)
        assert not any(qg.is_quad(s) for s in roles.values())
        if case["bm"]:                                                                    # the input is read through the row map, not copied
            assert qg.layer_calls(*layers[list(sg.LAYER_CASES).index(name)])[0].split()[7] == "1"
    assert sg.LAYER_CASES["bm_f100"]["expect"]["gemm_nn_xw"] == sg.nn_dma(6, 20)          # the standard first layer at 20 353 .. 65 535 rows
    assert {c["expect"]["gemm_tn_hc"] for c in sg.LAYER_CASES.values()} == {sg.tn_dma(2, 32), sg.tn_staged(1)}
    t, b, r = sg.BF3_DIMS
    assert r == t * b * 19
    for name, case in sg.BF3_CASES.items():
        assert case["h"] == 64 and sg.bf3_planned(plan_driver, case, r) == case["expect"], name
    assert {c["expect"]["gemm_nn_xw"] for c in sg.BF3_CASES.values()} == {sg.nn_bf3(12)}
    assert {c["expect"]["gemm_nn_dx"] for c in sg.BF3_CASES.values()} == {sg.nn_bf3(10), sg.nn_bf3(8), sg.nn_dma(2, 16)}


def test_case_table_covers_every_reachable_split_instance(plan_driver):
    """layers of 16 / 32 / 64 units x every supported hop count x input widths 4..516 x both layouts, dconv with O = 16..192, the
    decoder's projection with Dout = 4..256, 19 to 291 840 rows, no dev knobs: the split instances those calls are planned with are
    exactly the ones the tables name"""
    reachable = sg.reachable_instances(plan_driver)
    named = sg.named_instances()
    assert reachable == named, {"reachable without a case": sorted(reachable - named), "named but unreachable": sorted(named - reachable)}
    assert len(reachable) == 13           # seven gemm_nn_dma_kernel, two gemm_nn_kernel, three gemm_tn_dma_kernel, gemm_tn_kernel<1>
    # (a case that shares its instances with another one is still there for its edge: none leaves unnoticed)
    assert (len(sg.DCONV_CASES), len(sg.DCONV_SPARSE_CASES), len(sg.LAYER_CASES), len(sg.BF3_CASES), len(sg.KNOB_CASES)) == (13, 3, 3, 3, 9)


def test_dev_knob_instances_are_the_ones_the_emulator_twins_name(plan_driver):
    """the same sweep under knob 0 (staged NN), knob 1 (staged TN) and knob 14 (8-wave TN): what only a dev build reaches is what
    split_gemm_suite.KNOB_CASES names (run by tests/test_emu_parity.py) plus the three instances it says nobody runs"""
    product = sg.reachable_instances(plan_driver, widths=range(4, 132, 4))
    assert product == sg.named_instances()
    extra = set()
    for knobs in ({0: 1}, {1: 1}, {14: 48}):
        extra |= sg.reachable_instances(plan_driver, knobs=sg.knob_string(knobs), widths=range(4, 132, 4)) - product
    named = set()
    for name, (dims, knobs, expect) in sg.KNOB_CASES.items():
        assert dims[2] * dims[3] <= 304, name
        symbols, _ = sg.dconv_planned(plan_driver, [dims], cus=qg.EMU_CUS, knobs=sg.knob_string(knobs))[0]
        assert symbols == expect, (name, symbols)
        named |= set(expect.values()) - product
    assert extra == named | sg.KNOB_ONLY_NOT_RUN and not named & sg.KNOB_ONLY_NOT_RUN, (sorted(extra), sorted(named))
    assert len(extra) == 12


def test_compiled_but_unreachable(plan_driver):
    """gemm_nn(...) of csrc/api.cpp goes through run_nn_chunk<4>, which instantiates gemm_nn_kernel<4, 32 | 20 | 16 | 4> beside the DMA
    kernels it is there for.  No plan selects them: gemm_nn_plan picks NCTW = 4 (and 5) only `&& dma`, and a Dma plan never takes the
    staged branch -- neither in a product build nor under any NN knob, which is what this test holds.  They stay compiled: the switch
    in run_nn_chunk is the same for every NCTW, the four dead instances cost code-object bytes and nothing at run time, and taking
    them out would change how the product library is built for no test's benefit.  A rule change that starts to select one of
    them fails here and in the completeness checks above, which is the moment to give it a case."""
    found = sg.reachable_instances(plan_driver, widths=range(4, 132, 4)) | sg.reachable_instances(plan_driver, knobs=sg.knob_string({0: 1}), widths=range(4, 132, 4))
    staged = {s for s in found if s.startswith("gemm_nn_kernel<")}
    assert staged and not any(s.startswith(("gemm_nn_kernel<4,", "gemm_nn_kernel<5,")) for s in staged), sorted(staged)
    with open(os.path.join(qg.CSRC, "api.cpp")) as f:
        assert "run_nn_chunk<4>" in f.read()                                              # (still compiled: the statement above is about this tree)


def test_sparse_cotangent_clips():
    assert sg.dconv_sparse_clips(127, 19, 128) == [0, 6, 121, 126]       # row 128 = node 14 of clip 6; split 18 starts at row 2304 = clip 121
    assert sg.dconv_sparse_clips(1072, 19, 160) == [0, 8, 1069, 1071]    # 128 splits of 160 rows: the last starts at row 20 320


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sg.DCONV_CASES))
def test_split_gemm_dconv_case(hip_library, plan_driver, name):
    sg.check_dconv(name, "cuda", plan_driver, _cus())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sg.DCONV_SPARSE_CASES))
def test_split_gemm_dconv_case_sparse_cotangent(hip_library, plan_driver, name):
    sg.check_dconv(name, "cuda", plan_driver, _cus(), sparse=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sg.LAYER_CASES))
def test_split_gemm_layer_case(hip_library, name):
    assert sg.LAYER_DIMS[2] < 256 * _cus()                                                # (below the whole-block kernels on this device)
    sg.check_layer(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sg.BF3_CASES))
def test_split_gemm_bf16_split_case(hip_library, name):
    sg.check_bf3_layer(name, "cuda")
