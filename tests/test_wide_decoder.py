"""The persistent decoder kernels at outputs of 129..256 columns (time-domain SSL, input_dim = output_dim = 200): the backward's wide
tail (input-gradient tiles wave + 8 and wave + 12 from a second pass over the adjoint hop rows), the forward at 9..16 output tiles,
and what they enable -- teacher-forcing flags on the device and one captured graph under curriculum learning
(tests/wide_decoder_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again, marked `gpu`, on
the MI355X library.  On the commit before these kernels the capability rows that answer true answer false and every shape check
stops at its `decoder_is_persistent` assertion."""
import os

import pytest
import torch

import wide_decoder_suite as wd


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
def test_capability_table_emu(emulator):
    wd.check_capability_table()


@pytest.mark.parametrize("tag", list(wd.WIDE_SHAPES))
def test_wide_decoder_vs_oracle_emu(emulator, adj3d, tag):
    wd.check_wide_shape("cpu", adj3d, wd.WIDE_SHAPES[tag])


def test_model_device_curriculum_200_emu(emulator, adj3d):
    wd.check_model_device_curriculum("cpu", adj3d, dropout=0.5, reps=3)


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capability_table(hip_library):
    wd.check_capability_table()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(wd.WIDE_SHAPES))
def test_wide_decoder_vs_oracle(hip_library, adj3d, tag):
    wd.check_wide_shape("cuda", adj3d, wd.WIDE_SHAPES[tag])


@pytest.mark.gpu
def test_wide_decoder_vs_oracle_more_clips_than_workgroups(hip_library, adj3d):
    torch.set_num_threads(16)
    wd.check_wide_shape("cuda", adj3d, wd.MANY_CLIPS)


@pytest.mark.gpu
def test_persistent_kernels_ran(hip_library, adj3d):
    wd.check_persistent_kernels_ran("cuda", adj3d)


@pytest.mark.gpu
def test_curriculum_learning_replays_as_a_graph_200(hip_library):
    wd.check_curriculum_graph_replay("cuda", steps=6)


@pytest.mark.gpu
def test_model_device_curriculum_200(hip_library, adj3d):
    wd.check_model_device_curriculum("cuda", adj3d, dropout=0.5, reps=3)


@pytest.mark.gpu
def test_wide_decoder_is_deterministic(hip_library, adj3d):
    wd.check_determinism("cuda", adj3d, repeats=50)
