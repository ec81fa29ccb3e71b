"""Native-rate recordings resampled to 200 Hz on the device: `torch.ops.eeg_dcrnn.resample`, `resample_recording(s)`,
`RecordingDataset.from_native_rate` (tests/resample_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU)
and again, marked `gpu`, on the MI355X library; the largest length runs on the MI355X only."""
import os

import pytest
import torch

import resample_suite as rs


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


# ---- no library ----------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference():
    rs.check_golden()


def test_case_branches():
    rs.check_case_branches()


def test_cases_reach_every_pass_count():
    rs.check_plan_completeness()


def test_fake_implementation():
    rs.check_fake()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 19])
def test_cases_emu(emulator, channels):
    rs.check_cases("cpu", channels)


def test_pass_counts_emu(emulator):
    rs.check_pass_counts("cpu")          # (transforms up to 2^17 points: about a second on the emulator)


def test_invariance_emu(emulator):
    rs.check_invariance("cpu")


def test_layout_end_to_end_emu(emulator):
    rs.check_layout_end_to_end("cpu")


def test_refusals_emu(emulator):
    rs.check_refusals("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 19])
def test_cases(hip_library, channels):
    rs.check_cases("cuda", channels)


@pytest.mark.gpu
def test_pass_counts(hip_library):
    rs.check_pass_counts("cuda")


@pytest.mark.gpu
def test_largest(hip_library):
    rs.check_largest("cuda")


@pytest.mark.gpu
def test_invariance(hip_library):
    rs.check_invariance("cuda")


@pytest.mark.gpu
def test_layout_end_to_end(hip_library):
    rs.check_layout_end_to_end("cuda")


@pytest.mark.gpu
def test_refusals(hip_library):
    rs.check_refusals("cuda")
