"""The SSL evaluation pass on the device: `ops.ssl_eval_scores`, `ops.ssl_eval_metrics`, `TrainStep.ssl_evaluator` /
`DeviceSSLEvaluator` (tests/ssl_eval_suite.py).  Every check runs on the emulator build of the kernel sources (no GPU) and again,
marked `gpu`, on the MI355X library; the captured pass needs HIP graphs and runs on the GPU only; two gloo ranks run on the emulator."""
import os
import sys

import pytest
import torch

import ssl_eval_suite as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ["shared", "corr"]
NEW_GROUND = ["raw_fft", "time_domain"]


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
def test_scores_kernel_emu(emulator):
    se.check_scores_kernel("cpu")


def test_placement_independence_emu(emulator):
    se.check_placement_independence("cpu")


def test_record_emu(emulator):
    se.check_record("cpu")


@pytest.mark.parametrize("kind", PASSES)
def test_pass_emu(emulator, adj3d, kind):
    se.check_pass("cpu", adj3d, kind, units=16)


@pytest.mark.parametrize("kind", NEW_GROUND)
def test_new_ground_emu(emulator, adj3d, kind):
    se.check_new_ground("cpu", adj3d, kind, units=16)


def test_no_side_effects_emu(emulator, adj3d):
    se.check_no_side_effects("cpu", adj3d, units=16)


def test_refusals_emu(emulator, adj3d):
    se.check_refusals("cpu", adj3d)


def test_opcheck_emu(emulator):
    se.check_opcheck("cpu")


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
    out = {}
    for clips in (23, 19):
        st, ds, supports = se.two_rank_case(adj3d, clips)
        ev = st.ssl_evaluator(ds, se.B, supports=supports, keep_predictions=True)
        assert (ev.sampler.rank, ev.sampler.world, ev.sampler.steps_per_epoch) == (rank, world, 3)
        value = ev.run(capture=False)
        out[clips] = {"value": value, "scores": ev._scores.clone(), "record": ev.record.clone(), "clip_mae": ev.clip_mae.clone(),
                      "predictions": ev.predictions.clone(), "last_clip_w": ev.sampler.clip_w.clone()}
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_result(tmp_path, adj3d):
    """P = 23, B = 4, world = 2: three steps, rank r takes the slots cursor + 4r .. of each; the last step leaves rank 1 three clips
    (20, 21, 22).  The same with a pool of 19 clips: the last step leaves rank 1 EMPTY (every weight 0) and it still joins the
    all-reduce.  Every rank returns the single-process result of batch size 4: the (3, P) scores and the record bit for bit, the same
    float; the kept predictions are the rank's own slots, zeros elsewhere, and together they are the single process's."""
    import torch.multiprocessing as mp
    import emu_support
    emu_support.install_emulator()          # builds the emulator library once, before forking
    port = 34500 + (os.getpid() % 2000)
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2))
    for clips in (23, 19):
        st, ds, supports = se.two_rank_case(adj3d, clips)
        ev = st.ssl_evaluator(ds, se.B, supports=supports, keep_predictions=True)
        want = ev.run(capture=False)
        assert ev.result["batches"] == -(-clips // se.B)
        for r in (r0, r1):
            got = r[clips]
            assert got["value"] == want, (clips, got["value"], want)
            assert torch.equal(got["scores"], ev._scores) and torch.equal(got["record"], ev.record) and torch.equal(got["clip_mae"], ev.clip_mae)
        own0 = torch.zeros(clips, dtype=torch.bool)
        for start in range(0, clips, 2 * se.B):
            own0[start:start + se.B] = True
        assert torch.equal(r0[clips]["predictions"][own0], ev.predictions[own0]) and not bool(r0[clips]["predictions"][~own0].any())
        assert torch.equal(r1[clips]["predictions"][~own0], ev.predictions[~own0]) and not bool(r1[clips]["predictions"][own0].any())
    assert r1[19]["last_clip_w"].tolist() == [0.0] * 4 and r1[23]["last_clip_w"].tolist() == [1.0, 1.0, 1.0, 0.0]
    assert r0[19]["last_clip_w"].tolist() == [1.0, 1.0, 1.0, 0.0]
    emu_support.uninstall()


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scores_kernel(hip_library):
    se.check_scores_kernel("cuda")


@pytest.mark.gpu
def test_placement_independence(hip_library):
    se.check_placement_independence("cuda")


@pytest.mark.gpu
def test_record(hip_library):
    se.check_record("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PASSES)
def test_pass(hip_library, adj3d, kind):
    se.check_pass("cuda", adj3d, kind, units=64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NEW_GROUND)
def test_new_ground(hip_library, adj3d, kind):
    se.check_new_ground("cuda", adj3d, kind, units=64)


@pytest.mark.gpu
def test_no_side_effects(hip_library, adj3d):
    se.check_no_side_effects("cuda", adj3d, units=64)


@pytest.mark.gpu
def test_captured_pass_equals_eager(hip_library, adj3d):
    se.check_captured("cuda", adj3d)


@pytest.mark.gpu
def test_captured_pass_beside_training_graph(hip_library, adj3d):
    se.check_captured_beside_training_graph("cuda", adj3d)


@pytest.mark.gpu
def test_refusals(hip_library, adj3d):
    se.check_refusals("cuda", adj3d)


@pytest.mark.gpu
def test_opcheck(hip_library):
    se.check_opcheck("cuda")
