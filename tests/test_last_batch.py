"""An epoch that keeps its short last batch (`EpochSampler(..., drop_last=False)`): the validity gather, the per-clip weights in the
criterion kernels, the device increment of the curriculum counter, and `TrainStep.step_from` / `capture_epoch` / checkpointing with
such a sampler (tests/last_batch_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again, marked
`gpu`, on the MI355X library; the captured epoch needs HIP graphs and runs on the GPU only."""
import os

import pytest
import torch

import last_batch_suite as lb

MODES = ["detection", "classification", "ssl"]


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


def _units(mode):
    return 64 if mode == "detection" else 16     # (the spectral path: 64 units)


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_gather_validity_emu(emulator):
    lb.check_gather_validity("cpu")


def test_full_batch_is_unweighted_emu(emulator):
    lb.check_full_batch_is_unweighted("cpu")


def test_kept_clips_emu(emulator):
    lb.check_kept_clips("cpu")


@pytest.mark.parametrize("mode", MODES)
def test_invalid_slot_content_emu(emulator, adj3d, mode):
    lb.check_invalid_slot_content("cpu", adj3d, mode, units=_units(mode))


@pytest.mark.parametrize("mode", MODES)
def test_short_step_emu(emulator, adj3d, mode):
    lb.check_short_step("cpu", adj3d, mode, units=_units(mode))


def test_two_ranks_emu(emulator, adj3d):
    lb.check_two_ranks("cpu", adj3d, units=16)


def test_curriculum_counter_emu(emulator):
    lb.check_curriculum_counter("cpu")


def test_curriculum_step_emu(emulator, adj3d):
    lb.check_curriculum_step("cpu", adj3d)


def test_resume_emu(emulator, adj3d):
    lb.check_resume("cpu", adj3d, units=16)


def test_refusals_emu(emulator):
    lb.check_refusals("cpu")


def test_past_the_end_emu(emulator, adj3d):
    lb.check_past_the_end("cpu", adj3d, units=16)


def test_opcheck_emu(emulator):
    lb.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gather_validity(hip_library):
    lb.check_gather_validity("cuda")


@pytest.mark.gpu
def test_full_batch_is_unweighted(hip_library):
    lb.check_full_batch_is_unweighted("cuda")


@pytest.mark.gpu
def test_kept_clips(hip_library):
    lb.check_kept_clips("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_invalid_slot_content(hip_library, adj3d, mode):
    lb.check_invalid_slot_content("cuda", adj3d, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_short_step(hip_library, adj3d, mode):
    lb.check_short_step("cuda", adj3d, mode)


@pytest.mark.gpu
def test_two_ranks(hip_library, adj3d):
    lb.check_two_ranks("cuda", adj3d)


@pytest.mark.gpu
def test_curriculum_counter(hip_library):
    lb.check_curriculum_counter("cuda")


@pytest.mark.gpu
def test_curriculum_step(hip_library, adj3d):
    lb.check_curriculum_step("cuda", adj3d)


@pytest.mark.gpu
def test_resume(hip_library, adj3d):
    lb.check_resume("cuda", adj3d)


@pytest.mark.gpu
def test_captured_epoch_equals_eager(hip_library, adj3d):
    lb.check_captured_epoch("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library):
    lb.check_refusals("cuda")


@pytest.mark.gpu
def test_past_the_end(hip_library, adj3d):
    lb.check_past_the_end("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    lb.check_opcheck("cuda")
