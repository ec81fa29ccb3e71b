"""The scaler fit on the device: `ops.feature_moments`, `ops.moments_record`, `fit_scaler`, `TrainStep.fit_scaler`
(tests/scaler_fit_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again, marked `gpu`, on the
MI355X library; two gloo ranks run on the emulator."""
import os
import sys

import pytest
import torch

import scaler_fit_suite as sf

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
def test_reference_emu(emulator, golden_fft):
    sf.check_reference("cpu", golden_fft)


def test_features_emu(emulator):
    sf.check_features("cpu")


def test_placement_emu(emulator):
    sf.check_placement("cpu")


def test_bad_values_emu(emulator):
    sf.check_bad_values("cpu")


def test_record_emu(emulator):
    sf.check_record("cpu")


def test_passes_emu(emulator, adj3d):
    sf.check_passes("cpu", adj3d, units=16)


def test_refusals_emu(emulator, adj3d):
    sf.check_refusals("cpu", adj3d, units=16)


def test_opcheck_emu(emulator):
    sf.check_opcheck("cpu")


# ---- two gloo ranks on the emulator ----------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    torch.set_num_threads(1)
    import emu_support
    emu_support.install_emulator()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from eeg_gnn_ssl_amd import fit_scaler
    out = {}
    for clips in (7, 5):
        fit = fit_scaler(sf.two_rank_case(clips), 2, window=200)         # rank and world: the process group's
        out[clips] = {"mean": fit.mean, "std": fit.std, "count": fit.count, "scores": fit.scores.clone(), "record": fit.record.clone()}
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_result(tmp_path):
    """P = 7, B = 2, world = 2: two steps, rank r takes the slots cursor + 2r .. of each; the last step leaves rank 1 one clip (6).
    The same with a pool of 5 clips: the last step leaves rank 1 EMPTY (positions 6 and 7 lie behind the pool) and it still joins
    the all-reduce.  Every rank returns the single-process `ScalerFit`: the (4, P) scores and the record bit for bit, the same floats."""
    import torch.multiprocessing as mp
    import emu_support
    emu_support.install_emulator()          # builds the emulator library once, before forking
    from eeg_gnn_ssl_amd import fit_scaler
    port = 36500 + (os.getpid() % 2000)
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2))
    for clips in (7, 5):
        want = fit_scaler(sf.two_rank_case(clips), 2, window=200)
        assert want.clips == clips and want.count == (3 * clips - 1) * 4 * 100
        for r in (r0, r1):
            got = r[clips]
            assert (got["mean"], got["std"], got["count"]) == (want.mean, want.std, want.count), (clips, got, want)
            assert torch.equal(got["scores"], want.scores) and torch.equal(got["record"], want.record)
    emu_support.uninstall()


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference(hip_library, golden_fft):
    sf.check_reference("cuda", golden_fft)


@pytest.mark.gpu
def test_features(hip_library):
    sf.check_features("cuda")


@pytest.mark.gpu
def test_placement(hip_library):
    sf.check_placement("cuda")


@pytest.mark.gpu
def test_bad_values(hip_library):
    sf.check_bad_values("cuda")


@pytest.mark.gpu
def test_record(hip_library):
    sf.check_record("cuda")


@pytest.mark.gpu
def test_passes(hip_library, adj3d):
    sf.check_passes("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    sf.check_refusals("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_opcheck(hip_library):
    sf.check_opcheck("cuda")
