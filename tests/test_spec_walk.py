"""The spectral GEMMs where their rings, counted waits and persistent row ranges engage (tests/spec_walk_suite.py).

tests/spec_plan_suite.py runs every instance of the family, at 12 or 15 rows per frequency: one chunk per gemm_nnf_kernel workgroup, two
per gemm_tnf_kernel split, no whole tile in gemm_nng_kernel, no capped grid (test_product_cases_stay_shallow states the figures).  The
whole-model tests walk deeper, but only two gemm_nnf_kernel instances of five, and with dense cotangents over 10^5 rows, which do not
notice one row lost at a chunk edge.  This table runs ONE layer per case at row counts where the walk of every kernel, restated in
Python from the plan driver's grid, visits the states a change of ring, wait or range would touch.

Without a GPU: every case plans, at 256 CUs, the kernels it names, and the union of visited states over the table is exactly the
required list -- a rule change that moves an edge fails here until a case moves with it.  With one (`-m gpu`): each case and each sparse
twin against float64, with the walk restated for the device's own CU count.  The emulator twins are in tests/test_emu_parity.py."""
import os

import pytest
import torch

import quad_gemm_suite as qg
import spec_plan_suite as sp
import spec_walk_suite as sw


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
    torch.set_num_threads(16)             # (the float64 reference: 1-2 s per case)
    yield lib


# ---- no GPU: the table against the rules -----------------------------------------------------------------------------------------
def test_case_table_plans_what_it_names(plan_driver):
    """each case, at each of its row counts on 256 CUs, is planned as the kernels its `expect` names; B stays below the streamed BPTT
    kernel's batch; the twins likewise at the emulator's CU count"""
    for cases, cus in ((sw.CASES, sw.TABLE_CUS), (sw.TWINS, sp.EMU_CUS)):
        for name, per_rows in sw.table_walk(plan_driver, cases, cus).items():
            for t, b, must, _may, _visited, _notes in per_rows:
                assert b < 384 and must == cases[name]["expect"], (name, cus, t, b, must)
    for name in sw.SPARSE_CASES:
        assert name in sw.CASES
    assert sw.CASES["n19_f64_dx"]["dx"] and sw.CASES["n19_f64_dx"]["h0"] and sw.CASES["n19_f64_dx"]["lengths"] and sw.CASES["n19_f64_dx"]["k"] == 2
    assert {c["act"] for c in sw.CASES.values()} == {"tanh"}      # (spec_walk_suite.CASES: why no case runs relu)


def test_table_visits_every_required_state(plan_driver):
    """the union over the table of the states the restated walks visit at 256 CUs against REQUIRED, per instance"""
    visited = sw.union(sw.table_walk(plan_driver, sw.CASES, sw.TABLE_CUS))
    lost = sw.missing(visited, sw.REQUIRED)
    assert not lost, f"required (instance, state) pairs that no case visits at {sw.TABLE_CUS} CUs: {lost}"
    # every gemm_nnf / gemm_nng / gemm_tnf / grouped TN / gemm_dxf instance the product can reach is in the list
    reachable = {s for name in sp.PRODUCT_CASES for syms in sp.CASES[name]["expect"].values() for s in syms
                 if s.startswith(("gemm_nnf", "gemm_nng", "gemm_tnf", "gemm_tnq_grouped", "gemm_dxf"))}
    assert reachable == {inst.split(" [")[0] for inst in sw.REQUIRED if inst.startswith("gemm_")}
    # the wait ladder of gemm_nnf_kernel: what each PER takes at Q in {3, 4} (arms 14 and 8 need a deeper ring than kNnfNS = 3)
    arms = {}
    for name, per_rows in sw.table_walk(plan_driver, sw.CASES, sw.TABLE_CUS).items():
        case = sw.CASES[name]
        s = case["rows"][0]
        for kind, _, launches, _, _ in sw.plan_layer(plan_driver, case, *sw.pick_tb(s), sw.TABLE_CUS)[2]:
            if kind == "snn" and launches[0][0].startswith("gemm_nnf_kernel") and case["n"] == 19:
                arms[launches[0][0]] = sw.nnf_walk(case["fin"], s, sp.spec_rows(s), 19, launches[0][1])[2]
    assert arms == {sp.nnf(13): {7, 55, 63}, sp.nnf(9): {4, 52, 63}, sp.nnf(8, True): {4, 52, 63}, sp.nnf(5): {0, 48, 63}, sp.nnf(2): {0, 48, 63}}, arms


def test_twins_visit_their_states_at_the_emulators_cu_count(plan_driver):
    for name, per_rows in sw.table_walk(plan_driver, sw.TWINS, sp.EMU_CUS).items():
        lost = sw.missing(sw.union({name: per_rows}), sw.TWINS[name]["states"])
        assert not lost, (name, lost)


def test_product_cases_stay_shallow(plan_driver):
    """why this table exists: at 256 CUs the cases of spec_plan_suite.PRODUCT_CASES give every gemm_nnf_kernel workgroup ONE chunk, never
    form a gemm_nng_kernel tile of more than one row tile (a whole one has eight), and give every gemm_tnf_kernel split TWO chunks"""
    deep, per_instance = sw.product_depth(plan_driver)
    assert deep == {"gemm_nnf_kernel": 1, "gemm_nng_kernel": 1, "gemm_tnf_kernel": 2}, per_instance
    assert set(per_instance) == {sp.nnf(13), sp.nnf(9), sp.nnf(8, True), sp.nnf(5), sp.nnf(2), sp.nng(3), sp.nng(1), sp.tnf(1), sp.tnf(2), sp.tnf(3), sp.tnf(4)}
    assert all(q == deep[inst.split("<")[0]] for inst, q in per_instance.items()), per_instance


def test_walks_restate_the_worked_example(plan_driver):
    """S = 6120 rows of 19 nodes on 256 CUs, by hand: Sp = 6128, 96 chunks per frequency, 1824 chunks over 512 workgroups (Q in {3, 4});
    383 row tiles per group, 7277 over 512 workgroups; the fused TN at FXT >= 3 in 26 splits of 240 rows"""
    st, qs, arms = sw.nnf_walk(64, 6120, 6128, 19, 512)
    assert qs == {3: 224, 4: 288} and sum(q * c for q, c in qs.items()) == 1824 and st == sw.NNF_STATES
    st, tiles, q_max, longest = sw.nng_walk(132, 6128, 19, 512)
    assert sum(tiles.values()) == 512 and set(tiles) == {2, 3} and q_max == 27 and longest == 8
    _, _, calls = sw.plan_layer(plan_driver, sw.CASES["n19_f68"], 17, 360, 256)
    assert next(rest[:2] for kind, _, _, rest, _ in calls if kind == "stn") == [26, 240]
    assert sw.split_walk(6128, 26, 240, 8) == [30] * 25 + [16] and sw.split_walk(80, 2, 64, 8) == [8, 2]
    assert sw.sparse_clips(360, 240) == [0, 240, 359] and sw.sparse_clips(360, 480) == [0, 120, 359]
    assert [sw.nnf_per(k) for k in (100, 68, 64, 36, 12)] == [7, 5, 4, 3, 1]


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sw.CASES))
def test_spec_walk_case(hip_library, plan_driver, name):
    """(a CU count other than 256 that loses a state the case is there for fails with the missing states: it does not skip)"""
    sw.check_case(name, "cuda", plan_driver, _cus())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sw.SPARSE_CASES))
def test_spec_walk_case_sparse_cotangent(hip_library, plan_driver, name):
    """a cotangent on clip 0, the last clip and the clip that owns the first row of the second row split: the weight gradients against
    a few hundred rows' worth of signal, dX of every other clip exactly zero"""
    sw.check_case(name, "cuda", plan_driver, _cus(), sparse=True)
