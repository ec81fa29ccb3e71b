"""Class imbalance on the device: the multiplicative criteria, `ops.clip_weights`, `TrainStep(class_weights=, weight_norm=,
sample_weights=)` and `BalancedEpochSampler` (tests/class_weight_suite.py).  Every check runs on the emulator build of the kernel
sources (no GPU) and again, marked `gpu`, on the MI355X library; captured epochs need the GPU; two gloo ranks run on the emulator."""
import os
import sys

import pytest
import torch

import class_weight_suite as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def test_framework_emu(emulator):
    cw.check_framework("cpu")


def test_ones_are_free_emu(emulator):
    cw.check_ones_are_free("cpu")


def test_zero_selects_out_emu(emulator):
    cw.check_zero_selects_out("cpu")


def test_clip_weights_emu(emulator):
    cw.check_clip_weights("cpu")


def test_step_emu(emulator, adj3d):
    cw.check_step("cpu", adj3d, units=16)


def test_sampler_step_emu(emulator, adj3d):
    cw.check_sampler_step("cpu", adj3d, units=16)


def test_balanced_sampler_emu(emulator):
    cw.check_balanced_sampler("cpu")


def test_refusals_emu(emulator, adj3d):
    cw.check_refusals("cpu", adj3d, units=16)


def test_opcheck_emu(emulator):
    cw.check_opcheck("cpu")


# ---- two gloo ranks on the emulator ----------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir):
    import numpy as np
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    torch.set_num_threads(1)
    import emu_support
    emu_support.install_emulator()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    adj3d = np.load(os.path.join(ROOT, "tests", "golden", "adj_mx_3d.npy"))
    out = {norm: cw.two_rank_step("cpu", adj3d, dist.get_rank(), dist.get_world_size(), norm) for norm in ("sum", "count")}
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_average_to_the_single_process_step(tmp_path, adj3d):
    """the short last step of a drop_last=False epoch (7 clips left) with class weights, on two gloo ranks of B = 4 (4 + 3 clips) and
    on one process at B = 8: the mean of the ranks' losses and gradients -- what the summed all-reduce and its 1 / world leave -- is
    the single process's, at TOL, under both normalisations (every rank divides by the GLOBAL sum or count over world)."""
    import torch.multiprocessing as mp
    import emu_support
    emu_support.install_emulator()          # builds the emulator library once, before forking
    port = 36700 + (os.getpid() % 2000)
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    by_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2)]
    for norm in ("sum", "count"):
        cw.check_two_ranks_against("cpu", adj3d, [r[norm] for r in by_rank], norm)
    emu_support.uninstall()


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_framework(hip_library):
    cw.check_framework("cuda")


@pytest.mark.gpu
def test_ones_are_free(hip_library):
    cw.check_ones_are_free("cuda")


@pytest.mark.gpu
def test_zero_selects_out(hip_library):
    cw.check_zero_selects_out("cuda")


@pytest.mark.gpu
def test_clip_weights(hip_library):
    cw.check_clip_weights("cuda")


@pytest.mark.gpu
def test_step(hip_library, adj3d):
    cw.check_step("cuda", adj3d)


@pytest.mark.gpu
def test_sampler_step(hip_library, adj3d):
    cw.check_sampler_step("cuda", adj3d)


@pytest.mark.gpu
def test_captured_epoch(hip_library, adj3d):
    cw.check_captured_epoch("cuda", adj3d)


@pytest.mark.gpu
def test_two_ranks_on_one_device(hip_library, adj3d):
    for norm in ("sum", "count"):
        cw.check_two_ranks_against("cuda", adj3d, [cw.two_rank_step("cuda", adj3d, r, 2, norm, units=64) for r in range(2)], norm, units=64)


@pytest.mark.gpu
def test_balanced_sampler(hip_library):
    cw.check_balanced_sampler("cuda")


@pytest.mark.gpu
def test_balanced_captured(hip_library, adj3d):
    cw.check_balanced_captured("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    cw.check_refusals("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    cw.check_opcheck("cuda")
