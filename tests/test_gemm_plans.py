"""Which hoisted-GEMM kernel takes a shape (csrc/gemm_launch.h) is invisible to every parity test -- all generations of the kernels
give the same numbers -- and decides the speed of the general path.  tests/golden/gemm_plans_v1.json pins it: for a fixed list of
calls (the GEMM shapes of the benchmark workloads at 1 and 2 layers with the decoder's and dconv's, the emulator tests' shapes
with key 2 = 4, a seeded handful over all knobs) the plan that the selection code gave before it was gathered into that header:
kernel and template integers, grid, block, LDS bytes, row split, XCD placement, error.  A change of selection shows up here; where
it is wanted, the file is rewritten from the driver's own output (same call lines) and the commit says why."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "eeg_gnn_ssl_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_gemm_launch_plans_match_the_recorded_selection(tmp_path):
    with open(os.path.join(HERE, "golden", "gemm_plans_v1.json")) as f:
        plans = json.load(f)["plans"]
    assert len(plans) >= 300
    exe = str(tmp_path / "gemm_plan_driver")
    # the emulator's compiler and flags (tests/emu/build_emu.py): host code only, no kernel bodies behind gemm_launch.h
    subprocess.check_call([CLANG if os.path.exists(CLANG) else "clang++", "-x", "c++", "-std=c++17", "-O1", "-g", "-DEEG_PLATFORM_HEADER=\"platform_emu.h\"",
                           "-DEEG_DEV", "-I", os.path.join(HERE, "emu"), "-I", CSRC, "-Wno-unused-function", "-Wno-unknown-attributes",
                           os.path.join(HERE, "emu", "gemm_plan_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], input="".join(p["call"] + "\n" for p in plans), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(plans)
    wrong = [(p["call"], p["plan"], got) for p, got in zip(plans, out) if got != p["plan"]]
    assert not wrong, "%d of %d plans changed; first (call, recorded, now): %s" % (len(wrong), len(plans), wrong[:3])
