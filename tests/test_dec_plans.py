"""Which persistent decoder kernel takes a decoder (csrc/dec_launch.h) is invisible to every parity test -- the per-step launches give the
same numbers, dozens of times slower.  tests/golden/dec_plans_v1.json pins it: for a fixed list of calls (every hop count 1 .. 7 x 1 .. 5
layers x every output width 4 .. 264 at the last covered horizon, node count and the one covered hidden size; each of T = 65, N = 21 and
H = 32 alone at twenty of those shapes; clip counts on both sides of the grid's clamp; each dev knob and both) what the selection code
gave before it was gathered into that header: covered or not and, per direction, kernel symbol, grid, block and LDS bytes, or `per_step`.
A change of selection shows up here; where it is wanted, the file is rewritten from the driver's own output (same call lines) and the
commit says why.

tests/test_dec_kernels.py ties the plans to what runs: the driver against the restated rules of tests/dec_kernel_suite.py over its whole
grid, and every reachable instance proven through the event recorder, on the emulator and (`-m gpu`) on the MI355X."""
import json
import os
import subprocess

import pytest

import quad_gemm_suite as qg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "eeg_gnn_ssl_amd", "csrc")


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


def test_dec_launch_plans_match_the_recorded_selection(plan_driver):
    with open(os.path.join(HERE, "golden", "dec_plans_v1.json")) as f:
        plans = json.load(f)["plans"]
    assert len(plans) >= 2400 and sum(p["plan"].startswith("1 ;") for p in plans) >= 500
    out = subprocess.run([plan_driver], input="".join(p["call"] + "\n" for p in plans), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(plans)
    wrong = [(p["call"], p["plan"], got) for p, got in zip(plans, out) if got != p["plan"]]
    assert not wrong, "%d of %d plans changed; first (call, recorded, now): %s" % (len(wrong), len(plans), wrong[:3])


def test_dec_launch_header_is_host_code_on_its_own(tmp_path):
    """dec_launch.h alone, with the driver's compiler and flags: no kernel bodies, nothing but common.h and nnq_order.h"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "dec_launch.h"\nint main() { return eeg::dec_plan(eeg::DecCall{12, 40, 19, 64, 100, 3, 2}).covered ? 0 : 1; }\n')
    subprocess.check_call([qg.CLANG if os.path.exists(qg.CLANG) else "clang++", "-x", "c++", "-std=c++17", "-O1", "-DEEG_PLATFORM_HEADER=\"platform_emu.h\"",
                           "-DEEG_DEV", "-I", os.path.join(HERE, "emu"), "-I", CSRC, "-Wno-unused-function", "-Wno-unknown-attributes", "-fsyntax-only", str(src)])
    with open(os.path.join(CSRC, "dec_launch.h")) as f:
        text = f.read()
    assert "__global__" not in text
    assert sorted(ln.split('"')[1] for ln in text.splitlines() if ln.startswith("#include")) == ["common.h", "nnq_order.h"]
