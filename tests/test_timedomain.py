"""Time-domain inputs on the device (the reference without --use_fft): windowing + augmentation + scaler from raw signals, the
augmentation of ready windows, the correlation graph of wide channel rows, `TrainStep(use_fft=False)` (tests/timedomain_suite.py).
Every check runs on the emulator build of the kernel sources (no GPU) and again, marked `gpu`, on the MI355X library."""
import os

import pytest
import torch

import timedomain_suite as td

STEP_CASES = [(task, graph, raw) for task in ("detection", "classification", "ssl") for graph in ("distance", "correlation")
              for raw in (True, False)]


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


def test_oracle_chain_matches_the_reference_loaders():
    td.check_chain_vs_reference()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_window_features_emu(emulator):
    td.check_window_features("cpu")


def test_augment_windows_emu(emulator):
    td.check_augment_windows("cpu")


def test_corr_graph_rows_emu(emulator):
    td.check_corr_graph_rows("cpu", repeats=2)


def test_corr_graph_rows_long_emu(emulator):
    td.check_corr_graph_rows_long("cpu")


@pytest.mark.parametrize("task,graph,raw", STEP_CASES)
def test_timedomain_step_emu(emulator, adj3d, task, graph, raw):
    td.check_timedomain_step("cpu", adj3d, task=task, graph=graph, raw=raw, b=6, t_in=3, t_out=2)


def test_refusals_emu(emulator):
    td.check_refusals("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_features(hip_library):
    td.check_window_features("cuda")


@pytest.mark.gpu
def test_augment_windows(hip_library):
    td.check_augment_windows("cuda")


@pytest.mark.gpu
def test_corr_graph_rows(hip_library):
    td.check_corr_graph_rows("cuda", repeats=200)


@pytest.mark.gpu
def test_corr_graph_rows_long(hip_library):
    td.check_corr_graph_rows_long("cuda", b=8)


@pytest.mark.gpu
@pytest.mark.parametrize("task,graph,raw", STEP_CASES)
def test_timedomain_step(hip_library, adj3d, task, graph, raw):
    td.check_timedomain_step("cuda", adj3d, task=task, graph=graph, raw=raw, b=9, t_in=5, t_out=3)


@pytest.mark.gpu
def test_captured_timedomain_step_draws_afresh_at_every_replay(hip_library, adj3d):
    td.check_captured_timedomain_step("cuda", adj3d, b=6, t_in=3, t_out=2)


@pytest.mark.gpu
def test_timedomain_ssl_step_full_length(hip_library, adj3d):
    """60 s of raw input (12 000 samples per channel) and a 12 s raw target, dual random-walk correlation graph, the step checks'
    criteria; B = 16 keeps the CPU oracle well under a minute."""
    td.check_timedomain_step("cuda", adj3d, task="ssl", graph="correlation", raw=True, b=16, t_in=60, t_out=12)


@pytest.mark.gpu
def test_refusals(hip_library):
    td.check_refusals("cuda")
