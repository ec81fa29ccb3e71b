"""Variable-length clips in the raw-signal chain (the classification loader): length-aware featurisation, windowing and correlation
graphs, `TrainStep(padding_val=...)` (tests/varlen_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU)
and again, marked `gpu`, on the MI355X library."""
import os

import pytest
import torch

import varlen_suite as vl

# (graph, raw, use_fft, augment): every combination, and one with the step's own augmentation draws read back
STEP_CASES = [(graph, raw, use_fft, False) for graph in ("correlation", "distance") for raw in (True, False) for use_fft in (True, False)]
STEP_CASES.append(("correlation", True, True, True))


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


def test_oracle_chain_matches_the_reference_classification_loader():
    vl.check_chain_vs_reference()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_fft_features_len_emu(emulator):
    vl.check_fft_features_len("cpu")


def test_window_features_len_emu(emulator):
    vl.check_window_features_len("cpu")


@pytest.mark.parametrize("nodes", [4, 19, 32])
def test_graphs_len_emu(emulator, nodes):
    vl.check_graphs_len("cpu", nodes=(nodes,))


@pytest.mark.parametrize("graph,raw,use_fft,augment", STEP_CASES)
def test_varlen_step_emu(emulator, adj3d, graph, raw, use_fft, augment):
    vl.check_varlen_step("cpu", adj3d, graph=graph, raw=raw, use_fft=use_fft, augment=augment, b=4, t_len=3)


def test_refusals_emu(emulator):
    vl.check_refusals("cpu")


def test_opcheck_emu(emulator):
    vl.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fft_features_len(hip_library):
    vl.check_fft_features_len("cuda")


@pytest.mark.gpu
def test_window_features_len(hip_library):
    vl.check_window_features_len("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", [4, 19, 32])
def test_graphs_len(hip_library, nodes):
    vl.check_graphs_len("cuda", nodes=(nodes,))


@pytest.mark.gpu
@pytest.mark.parametrize("graph,raw,use_fft,augment", STEP_CASES)
def test_varlen_step(hip_library, adj3d, graph, raw, use_fft, augment):
    vl.check_varlen_step("cuda", adj3d, graph=graph, raw=raw, use_fft=use_fft, augment=augment, b=6, t_len=4)


@pytest.mark.gpu
def test_captured_varlen_step_replays_with_refilled_lengths(hip_library, adj3d):
    vl.check_captured_varlen_step("cuda", adj3d, b=6, t_len=4)


@pytest.mark.gpu
def test_refusals(hip_library):
    vl.check_refusals("cuda")


@pytest.mark.gpu
def test_opcheck(hip_library):
    vl.check_opcheck("cuda")
