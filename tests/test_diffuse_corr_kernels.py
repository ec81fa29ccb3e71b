"""The hop-diffusion and correlation-Gram kernels at every template instance a call reaches (tests/diffuse_corr_suite.py): one tiny
operator call per instance with the event recorder on -- the call must launch exactly the planned symbol under its role -- and its
result against a float64 restatement, with the helpers and tolerances the parity suites apply to the same operators.  All 43
instances are reachable without a dev knob (tests/test_diffuse_corr_plans.py proves it against the plan driver), so the same cases
run on the emulator and (`-m gpu`) on the product library; none is skipped."""
import os

import pytest
import torch

import diffuse_corr_suite as dc


@pytest.fixture
def emulator():
    import emu_support
    lib = emu_support.install_emulator()
    yield lib
    emu_support.uninstall()


@pytest.fixture
def hip_library():
    from eeg_gnn_ssl_amd import _lib
    _lib._LIB = None
    lib = _lib.get_lib()                  # ImportError if the HIP library is missing: no fallback
    assert lib.is_device_build and os.path.basename(lib.path) == "libeeg_dcrnn_hip.so"
    assert torch.cuda.is_available()
    yield lib


@pytest.mark.parametrize("name", list(dc.DIFFUSE_CASES))
def test_diffusion_case_emu(emulator, name):
    dc.check_diffuse_case(name, "cpu")


@pytest.mark.parametrize("name", list(dc.CORR_CASES))
def test_gram_case_emu(emulator, name):
    dc.check_corr_case(name, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.DIFFUSE_CASES))
def test_diffusion_case(hip_library, name):
    dc.check_diffuse_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.CORR_CASES))
def test_gram_case(hip_library, name):
    dc.check_corr_case(name, "cuda")
