"""Which kernel of the spectral form takes a call (csrc/spec_launch.h) is invisible to every parity test -- the grouped kernels give the
same numbers as the fused ones -- and decides the speed of the metric's configuration.  tests/golden/spec_plans_v1.json pins it: for a
fixed list of calls (every spectral launch of cfg2 / cfg4, the time-domain and SSL layer-0 widths, the widths 4 .. 132 and the node counts
of the randomized GPU test on both sides of every rule edge, row counts where the split clamps, two CU counts, each dev knob) the launch
that the selection code gave before it was gathered into that header: kernel symbol, grid, block, LDS bytes, row splits, partial sizes.
A change of selection shows up here; where it is wanted, the file is rewritten from the driver's own output (same call lines) and the
commit says why.

tests/spec_plan_suite.py ties the plans to what runs: its case table must plan exactly the kernel instances the rules can reach (here,
without a GPU), and each case proves through the event recorder that the planned kernels took its launches (`-m gpu` below for the
MI355X library; tests/test_emu_parity.py for the emulator, which also runs the cases under dev knobs)."""
import json
import os
import subprocess

import pytest
import torch

import quad_gemm_suite as qg
import spec_plan_suite as sp

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "eeg_gnn_ssl_amd", "csrc")


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
    yield lib


# ---- no GPU ---------------------------------------------------------------------------------------------------------------------
def test_spec_launch_plans_match_the_recorded_selection(plan_driver):
    with open(os.path.join(HERE, "golden", "spec_plans_v1.json")) as f:
        plans = json.load(f)["plans"]
    assert len(plans) >= 2000
    out = subprocess.run([plan_driver], input="".join(p["call"] + "\n" for p in plans), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(plans)
    wrong = [(p["call"], p["plan"], got) for p, got in zip(plans, out) if got != p["plan"]]
    assert not wrong, "%d of %d plans changed; first (call, recorded, now): %s" % (len(wrong), len(plans), wrong[:3])


def test_spec_launch_header_is_host_code_on_its_own(tmp_path):
    """spec_launch.h alone, with the driver's compiler and flags: no kernel bodies, nothing but common.h, nnq_order.h and spec_common.h"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "spec_launch.h"\nint main() { return eeg::spec_supported(3, 4, 19, 64, 100, 3, 0) ? 0 : 1; }\n')
    subprocess.check_call([qg.CLANG if os.path.exists(qg.CLANG) else "clang++", "-x", "c++", "-std=c++17", "-O1", "-DEEG_PLATFORM_HEADER=\"platform_emu.h\"",
                           "-DEEG_DEV", "-I", os.path.join(HERE, "emu"), "-I", CSRC, "-Wno-unused-function", "-Wno-unknown-attributes", "-fsyntax-only", str(src)])
    with open(os.path.join(CSRC, "spec_launch.h")) as f:
        text = f.read()
    assert "__global__" not in text
    assert sorted(ln.split('"')[1] for ln in text.splitlines() if ln.startswith("#include")) == ["common.h", "nnq_order.h", "spec_common.h"]


def test_case_table_plans_what_it_names(plan_driver):
    """each case is planned by spec_launch.h, at 256 CUs and at the emulator's 4, as the kernels its `expect` names"""
    for cus in (256, sp.EMU_CUS):
        models = [(c["n"], c["din"], 2, sp.T_LEN, c["b"], cus, c["knobs"]) for c in sp.CASES.values()]
        for (name, case), (must, _) in zip(sp.CASES.items(), sp.planned(plan_driver, models)):
            assert must == case["expect"], (name, cus, must)
    for case in sp.CASES.values():            # pad rows in every frequency
        assert (sp.T_LEN * case["b"]) % 16 != 0


def test_case_table_covers_every_reachable_spectral_instance(plan_driver):
    """2 .. 32 nodes x every supported input width, no knobs / each knob / all three: the kernel instances those models are planned with
    are exactly the ones the case table plans -- a rule change that reaches another instance fails here until a case runs it"""
    reachable = sp.reachable_instances(plan_driver)
    models = [(c["n"], c["din"], 2, sp.T_LEN, c["b"], 256, c["knobs"]) for c in sp.CASES.values()]
    table = {s for must, may in sp.planned(plan_driver, models) for roles in (must, may) for syms in roles.values() for s in syms}
    assert reachable == table, {"reachable without a case": sorted(reachable - table), "planned by the table only": sorted(table - reachable)}
    named = {s for case in sp.CASES.values() for syms in case["expect"].values() for s in syms}
    # every instance but the to-node MFMA mixes of the 192-wide operands is a launch that a case MUST record
    assert table - named <= {sp.mix_mfma(0, 10), sp.mix_mfma(0, 16), sp.mix_mfma(1, 10), sp.mix_mfma(1, 16)} and named <= table
    assert len(reachable) == 23           # 5 nnf, 2 nng, 4 tnf, 3 grouped TN + the pair, 2 dxf, 4 MFMA mixes, the 19-node and the generic mix
    # without knobs (the product build) the planar grouped TN kernel is the one instance out of reach
    product = [(c["n"], c["din"], 2, sp.T_LEN, c["b"], 256, c["knobs"]) for name, c in sp.CASES.items() if name in sp.PRODUCT_CASES]
    in_product = {s for must, may in sp.planned(plan_driver, product) for roles in (must, may) for syms in roles.values() for s in syms}
    assert table - in_product == {sp.tng(2, True)}


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sp.PRODUCT_CASES))
def test_spectral_case_runs_the_planned_kernels(hip_library, plan_driver, adj3d, name):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sp.check_case(name, "cuda", adj3d, plan_driver, cus)
