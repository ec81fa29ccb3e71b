"""The persistent whole-block GEMMs (csrc/kernels_gemm_q.h) at every template instance a product build can reach, each pinned on the
MI355X by one single-layer case with just over 256 rows per CU against a float64 reference (tests/quad_gemm_suite.py).

Without a GPU: the plan driver enumerates the instances that the selection rules of csrc/gemm_launch.h can hand a layer, and the case
table must plan exactly that set -- a rule change that makes another instance reachable fails here until a case runs it.  With one
(`-m gpu`): every case proves through the event recorder that the kernels it names took its GEMMs, then compares the hidden sequence
and all gradients; three cases run again with a cotangent on three clips only, which measures a row lost or doubled at a split or
tile boundary against a few hundred rows instead of 65 thousand.  The emulator twin of the table is in tests/test_emu_parity.py."""
import os

import pytest
import torch

import quad_gemm_suite as qg

TABLE_CUS = 256                       # the CU count the table's plans are stated for (MI355X); the selection does not depend on it


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


# ---- no GPU: the table against the selection rules -------------------------------------------------------------------------------
def test_case_table_plans_what_it_names(plan_driver):
    """each case, at the row count it gets on a 256-CU device, is planned by gemm_launch.h as the kernels its `expect` names"""
    rows_min = 256 * TABLE_CUS
    layers, dims = [], {}
    for name, case in qg.CASES.items():
        t, b, r = qg.case_dims(case, rows_min)
        assert r >= rows_min and r % case["rows"][0] == case["rows"][1] and b < 384, (name, t, b, r)
        dims[name] = (t, b, r)
        layers.append((case["h"], qg.hops(case), case["fin"], r, case["bm"], TABLE_CUS))
    for (name, case), (roles, _) in zip(qg.CASES.items(), qg.planned(plan_driver, layers)):
        assert roles == case["expect"], (name, dims[name], roles)
    # the edges the table is there for
    assert dims["at_threshold"][2] == rows_min
    assert dims["ragged_128"][2] % 16 == 0 and dims["ragged_128"][2] % 128 == 48
    assert dims["ragged_16"][2] % 16 == 6 and not any(qg.is_quad(s) for r, s in qg.CASES["ragged_16"]["expect"].items() if r.startswith("gemm_tn"))
    assert sum(case["h0"] for case in qg.CASES.values()) >= 2 and any(case["lengths"] for case in qg.CASES.values())
    assert {case["act"] for case in qg.CASES.values()} == {"tanh", "relu"}


def test_case_table_covers_every_reachable_quad_instance(plan_driver):
    """16 / 32 / 64 units x every supported hop count x input widths 4..516 x both layouts at 256 rows per CU, no dev knobs: the quad
    instances those layers are planned with are exactly the ones the case table names"""
    reachable = qg.reachable_instances(plan_driver, TABLE_CUS)
    named = {s for case in qg.CASES.values() for s in case["expect"].values() if qg.is_quad(s)}
    assert reachable == named, {"reachable without a case": sorted(reachable - named), "named but unreachable": sorted(named - reachable)}
    assert len(reachable) == 16           # gemm_nnr_kernel<4, 2>, thirteen gemm_tnq_kernel instances, the two pair kernels


def test_sparse_cotangent_clips_straddle_the_first_split_boundary():
    assert qg.sparse_clips(288, 19, 144) == [0, 7, 287]          # row 144 = node 11 of clip 7 at step 0: rows 133..151
    assert qg.sparse_clips(217, 19, 528) == [0, 27, 216]
    assert qg.sparse_clips(5, 19, 19 * 7) == [0, 2, 4]           # second step: clip (7 mod 5)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
def _device_rows():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 256 * cus, cus


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(qg.CASES))
def test_quad_gemm_case(hip_library, plan_driver, name):
    rows_min, cus = _device_rows()
    qg.check_case(name, "cuda", rows_min, cus=cus, exe=plan_driver)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(qg.SPARSE_CASES))
def test_quad_gemm_case_sparse_cotangent(hip_library, plan_driver, name):
    rows_min, cus = _device_rows()
    qg.check_case(name, "cuda", rows_min, cus=cus, exe=plan_driver, sparse=True)
