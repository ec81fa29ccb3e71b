"""Occlusion maps on the device: `ops.occlude_expand`, `ops.occlusion_scores`, `occlusion_maps` / `TrainStep.occlusion_maps`
(tests/occlusion_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU, 16 units) and again, marked `gpu`,
on the MI355X library (64 units: the spectral form where the graph is shared)."""
import os

import pytest
import torch

import occlusion_suite as oc

CASES = sorted(oc.MAP_CASES)
STEP_KINDS = ["raw_fft", "time_domain"]


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
def test_expand_kernel_emu(emulator):
    oc.check_expand_kernel("cpu")


def test_scores_kernel_emu(emulator):
    oc.check_scores_kernel("cpu")


@pytest.mark.parametrize("name", CASES)
def test_maps_emu(emulator, adj3d, name):
    oc.check_maps("cpu", adj3d, name, units=16)


def test_prefix_sharing_emu(emulator, adj3d):
    oc.check_prefix_sharing("cpu", adj3d, units=16)


@pytest.mark.parametrize("kind", STEP_KINDS)
def test_train_step_emu(emulator, kind):
    oc.check_train_step("cpu", kind, units=16)


def test_no_side_effects_emu(emulator, adj3d):
    oc.check_no_side_effects("cpu", adj3d, units=16)


def test_refusals_emu(emulator, adj3d):
    oc.check_refusals("cpu", adj3d)


def test_opcheck_emu(emulator):
    oc.check_opcheck("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_expand_kernel(hip_library):
    oc.check_expand_kernel("cuda")


@pytest.mark.gpu
def test_scores_kernel(hip_library):
    oc.check_scores_kernel("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_maps(hip_library, adj3d, name):
    oc.check_maps("cuda", adj3d, name, units=64)


@pytest.mark.gpu
def test_prefix_sharing(hip_library, adj3d):
    oc.check_prefix_sharing("cuda", adj3d, units=64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STEP_KINDS)
def test_train_step(hip_library, kind):
    oc.check_train_step("cuda", kind, units=64)


@pytest.mark.gpu
def test_no_side_effects(hip_library, adj3d):
    oc.check_no_side_effects("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    oc.check_refusals("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    oc.check_opcheck("cuda")
