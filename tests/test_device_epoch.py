"""Epochs from a device-resident data set: the batch gather through a device-resident permutation and cursor, the epoch's shuffle,
`DeviceDataset` / `EpochSampler`, `TrainStep.step_from` / `capture_epoch` / `begin_epoch` and checkpointing
(tests/device_epoch_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again, marked `gpu`, on
the MI355X library; the captured epoch needs HIP graphs and runs on the GPU only."""
import os

import pytest
import torch

import device_epoch_suite as de

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


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_gather_equals_indexing_emu(emulator):
    de.check_gather("cpu")


def test_keys_and_permutation_emu(emulator):
    de.check_keys_and_permutation("cpu")


def test_epoch_coverage_emu(emulator):
    de.check_epoch_coverage("cpu")


def test_evaluation_from_batches_emu(emulator, adj3d):
    de.check_evaluation_from_batches("cpu", adj3d, units=16)


@pytest.mark.parametrize("mode", MODES)
def test_step_from_emu(emulator, adj3d, mode):
    de.check_step_from("cpu", adj3d, mode, units=64 if mode == "detection" else 16)     # (the spectral path: 64 units)


def test_resume_emu(emulator, adj3d):
    de.check_resume("cpu", adj3d, units=16)


def test_refusals_emu(emulator, adj3d):
    de.check_refusals("cpu", adj3d)


def test_opcheck_emu(emulator):
    de.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gather_equals_indexing(hip_library):
    de.check_gather("cuda")


@pytest.mark.gpu
def test_keys_and_permutation(hip_library):
    de.check_keys_and_permutation("cuda")


@pytest.mark.gpu
def test_epoch_coverage(hip_library):
    de.check_epoch_coverage("cuda")


@pytest.mark.gpu
def test_evaluation_from_batches(hip_library, adj3d):
    de.check_evaluation_from_batches("cuda", adj3d)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_step_from(hip_library, adj3d, mode):
    de.check_step_from("cuda", adj3d, mode)


@pytest.mark.gpu
def test_captured_epoch_equals_eager(hip_library, adj3d):
    de.check_captured_epoch("cuda", adj3d)


@pytest.mark.gpu
def test_resume(hip_library, adj3d):
    de.check_resume("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    de.check_refusals("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    de.check_opcheck("cuda")
