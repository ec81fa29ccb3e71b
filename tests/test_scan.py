"""Whole-recording scans on the device: `clip_table_scan` / `clip_labels_detection` / `annotation_bins`, `ops.scan_timeline`,
`ops.scan_events`, `ops.event_scores`, `TrainStep.scanner` (tests/scan_suite.py).  Every check runs on the emulator build of the kernel
sources (no GPU) and again, marked `gpu`, on the MI355X library; two gloo ranks and the hostile-table check run on the emulator."""
import os
import sys

import pytest
import torch

import scan_suite as ss

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


def test_builders():
    ss.check_builders()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_timeline_emu(emulator):
    ss.check_timeline("cpu")


def test_events_rules_emu(emulator):
    ss.check_events_rules("cpu")


def test_events_random_emu(emulator):
    ss.check_events_random("cpu")


def test_overflow_emu(emulator):
    ss.check_overflow("cpu")


def test_scores_emu(emulator):
    ss.check_scores("cpu")


@pytest.mark.parametrize("kind", ["detection", "detection_shared"])
def test_pass_emu(emulator, adj3d, kind):
    ss.check_pass("cpu", adj3d, kind, units=16)


def test_refusals_emu(emulator, adj3d):
    ss.check_refusals("cpu", adj3d, units=16)


def test_hostile_tables_emu(emulator):
    ss.check_hostile_tables()


def test_opcheck_emu(emulator):
    ss.check_opcheck("cpu")


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
    res = ss.two_rank_result()                                           # rank and world: the process group's
    torch.save({k: getattr(res, k).clone() for k in ss.RESULT_FIELDS} | {"scores": dict(res.scores)}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_result(tmp_path):
    """P = 8 windows, B = 3, world = 2: two steps, rank r takes the slots cursor + 3r .. of each; the last step leaves rank 0 two
    windows and rank 1 none, and it still joins the all-reduce.  Every rank returns the single-process `ScanResult` bit for bit."""
    import torch.multiprocessing as mp
    import emu_support
    emu_support.install_emulator()          # builds the emulator library once, before forking
    port = 37500 + (os.getpid() % 2000)
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    want = ss.two_rank_result(rank=0, world=1)
    assert int(want.record[1]) >= 0 and tuple(want.clip_probs.shape) == (8,)
    for r in range(2):
        got = torch.load(tmp_path / f"r{r}.pt", weights_only=False)
        for k in ss.RESULT_FIELDS:
            assert torch.equal(got[k], getattr(want, k)), (r, k)
        assert str(got["scores"]) == str(dict(want.scores))
    emu_support.uninstall()


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timeline(hip_library):
    ss.check_timeline("cuda")


@pytest.mark.gpu
def test_events_rules(hip_library):
    ss.check_events_rules("cuda")


@pytest.mark.gpu
def test_events_random(hip_library):
    ss.check_events_random("cuda")


@pytest.mark.gpu
def test_overflow(hip_library):
    ss.check_overflow("cuda")


@pytest.mark.gpu
def test_scores(hip_library):
    ss.check_scores("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["detection", "detection_shared"])
def test_pass(hip_library, adj3d, kind):
    ss.check_pass("cuda", adj3d, kind, units=64)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    ss.check_refusals("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_opcheck(hip_library):
    ss.check_opcheck("cuda")
