"""Clips cut out of device-resident recordings through a device clip table: `ops.gather_records`, `RecordingDataset`, the three
`clip_table_*` builders, and `TrainStep.step_from` / `capture_epoch` / `evaluator` / `ssl_evaluator` / checkpointing on top of them
(tests/record_pool_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again, marked `gpu`, on the
MI355X library; the captured epoch needs HIP graphs and runs on the GPU only, the table builders need neither."""
import os

import pytest
import torch

import record_pool_suite as rp

STEP_KINDS = ["detection", "detection_shared", "classification", "ssl", "timedomain"]
# every kind with the default sampler, and the epoch's short last step on the supervised and the SSL criterion
STEP_CASES = [(k, True) for k in STEP_KINDS] + [("classification", False), ("ssl", False)]


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


def test_table_builders():
    rp.check_builders()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_gather_equals_slicing_emu(emulator):
    rp.check_gather("cpu")


def test_hostile_tables_emu(emulator):
    rp.check_hostile_tables("cpu", everything=True)


@pytest.mark.parametrize("kind,drop_last", STEP_CASES)
def test_step_from_recordings_emu(emulator, adj3d, kind, drop_last):
    rp.check_step("cpu", adj3d, kind, drop_last, units=16)


def test_evaluators_emu(emulator, adj3d):
    rp.check_evaluators("cpu", adj3d, units=16)


def test_resume_emu(emulator, adj3d):
    rp.check_resume("cpu", adj3d, units=16)


def test_refusals_emu(emulator, adj3d):
    rp.check_refusals("cpu", adj3d)


def test_opcheck_emu(emulator):
    rp.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gather_equals_slicing(hip_library):
    rp.check_gather("cuda")


@pytest.mark.gpu
def test_hostile_tables(hip_library):
    rp.check_hostile_tables("cuda", everything=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,drop_last", STEP_CASES)
def test_step_from_recordings(hip_library, adj3d, kind, drop_last):
    rp.check_step("cuda", adj3d, kind, drop_last)


@pytest.mark.gpu
def test_captured_epoch_equals_eager(hip_library, adj3d):
    rp.check_captured_epoch("cuda", adj3d)


@pytest.mark.gpu
def test_evaluators(hip_library, adj3d):
    rp.check_evaluators("cuda", adj3d)


@pytest.mark.gpu
def test_resume(hip_library, adj3d):
    rp.check_resume("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    rp.check_refusals("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    rp.check_opcheck("cuda")
