"""The clustered bootstrap of the scores on the device: `ops.boot_counts` / `ops.boot_detection` / `ops.boot_classification` /
`ops.boot_records`, `bootstrap_scores`, `paired_difference`, `DeviceEvaluator.bootstrap`, `ScanResult.bootstrap`,
`RecordingDataset.clip_groups` (tests/boot_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again,
marked `gpu`, on the MI355X library."""
import os

import pytest
import torch

import boot_suite as bs


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
def test_counts_emu(emulator):
    bs.check_counts("cpu")


def test_detection_emu(emulator):
    bs.check_detection("cpu")


def test_tie_to_evaluator_emu(emulator):
    bs.check_tie_to_evaluator("cpu")


def test_classification_emu(emulator):
    bs.check_classification("cpu")


def test_records_emu(emulator):
    bs.check_records("cpu")


def test_intervals_emu(emulator):
    bs.check_intervals("cpu")


def test_undefined_emu(emulator):
    bs.check_undefined("cpu")


def test_evaluator_emu(emulator, adj3d):
    bs.check_evaluator("cpu", adj3d, units=16)


def test_scan_and_groups_emu(emulator, adj3d):
    bs.check_scan_and_groups("cpu", adj3d)


def test_refusals_emu(emulator):
    bs.check_refusals("cpu")


def test_opcheck_emu(emulator):
    bs.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_counts(hip_library):
    bs.check_counts("cuda")


@pytest.mark.gpu
def test_detection(hip_library):
    bs.check_detection("cuda")


@pytest.mark.gpu
def test_tie_to_evaluator(hip_library):
    bs.check_tie_to_evaluator("cuda")


@pytest.mark.gpu
def test_classification(hip_library):
    bs.check_classification("cuda")


@pytest.mark.gpu
def test_records(hip_library):
    bs.check_records("cuda")


@pytest.mark.gpu
def test_intervals(hip_library):
    bs.check_intervals("cuda")


@pytest.mark.gpu
def test_undefined(hip_library):
    bs.check_undefined("cuda")


@pytest.mark.gpu
def test_evaluator(hip_library, adj3d):
    bs.check_evaluator("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_scan_and_groups(hip_library, adj3d):
    bs.check_scan_and_groups("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library):
    bs.check_refusals("cuda")


@pytest.mark.gpu
def test_opcheck(hip_library):
    bs.check_opcheck("cuda")
