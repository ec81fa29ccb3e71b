"""The data side of the SSL step: paired featurisation, paired augmentation of features, `TrainStep(task="ssl")` with raw
targets and `data_augment`, capture / replay (tests/ssl_chain_suite.py).  Every check runs on the emulator build of the kernel
sources (no GPU) and again, marked `gpu`, on the MI355X library."""
import os

import pytest
import torch

import ssl_chain_suite as sc

STEP_CASES = [("distance", True), ("distance", False), ("correlation", True), ("correlation", False)]


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


def test_oracle_pair_chain_matches_the_reference_loader():
    sc.check_oracle_pair_vs_reference()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
def test_fft_features_pair_emu(emulator):
    sc.check_fft_features_pair("cpu")


def test_augment_features_emu(emulator):
    sc.check_augment_features("cpu")


@pytest.mark.parametrize("graph,raw", STEP_CASES)
def test_augmented_ssl_step_emu(emulator, adj3d, graph, raw):
    sc.check_augmented_ssl_step("cpu", adj3d, graph=graph, raw=raw, b=6, t_in=3, t_out=2)


@pytest.mark.parametrize("raw", [True, False])
def test_augmented_ssl_step_teacher_forced_emu(emulator, adj3d, raw):
    sc.check_augmented_ssl_step("cpu", adj3d, graph="correlation", raw=raw, b=6, t_in=2, t_out=3, curriculum=True)


def test_refusals_emu(emulator):
    sc.check_refusals("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fft_features_pair(hip_library):
    sc.check_fft_features_pair("cuda")


@pytest.mark.gpu
def test_augment_features(hip_library):
    sc.check_augment_features("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("graph,raw", STEP_CASES)
def test_augmented_ssl_step(hip_library, adj3d, graph, raw):
    sc.check_augmented_ssl_step("cuda", adj3d, graph=graph, raw=raw, b=9, t_in=5, t_out=3)


@pytest.mark.gpu
@pytest.mark.parametrize("raw", [True, False])
def test_augmented_ssl_step_teacher_forced(hip_library, adj3d, raw):
    sc.check_augmented_ssl_step("cuda", adj3d, graph="correlation", raw=raw, b=9, t_in=4, t_out=3, curriculum=True)


@pytest.mark.gpu
def test_captured_paired_step_draws_afresh_at_every_replay(hip_library, adj3d):
    sc.check_captured_ssl_step("cuda", adj3d, b=6, t_in=3, t_out=2)


@pytest.mark.gpu
def test_refusals(hip_library):
    sc.check_refusals("cuda")


@pytest.mark.gpu
def test_ssl_full_size_three_layers_distance_graph_spectral_vs_oracle():
    """The reference's SSL default (`--num_rnn_layers 3`) on the DISTANCE graph at full per-GPU size: B = 512, 60 s in / 12 s out,
    features, no augmentation, the scaled Laplacian handed in as ONE 2-D tensor.  Loss and every parameter gradient against the
    oracle (relative 1e-4, the criterion of `test_ssl_full_size_three_layers_vs_oracle`), AND the path: `ops.spectral_layer_calls`
    advanced by 3 -- the encoder's layers took the spectral form (the decoder runs its M = 3 kernels)."""
    import bench
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, ops, utils
    from oracle import dcrnn_oracle as orc
    dev = "cuda"
    task, _, t_len, batch, classes = bench.WORKLOADS["cfg5"]
    filt = "laplacian"
    x, y, lengths, sup = bench.synthetic_batch(task, filt, t_len, batch, classes, seed=8)
    assert x.shape == (512, 60, 19, 100) and y.shape == (512, 12, 19, 100) and len(sup) == 1
    shared = sup[0][0].contiguous() if sup[0].dim() == 3 else sup[0]
    assert shared.shape == (19, 19)
    torch.manual_seed(12)
    model = DCRNNModel_nextTimePred(bench.make_args(filt, layers=3), device=dev).to(dev).train()
    assert model.decoder.decoding_cells[1] is model.decoder.decoding_cells[2]
    before = ops.spectral_layer_calls
    pred = model(x.to(dev), y.to(dev), [shared.to(dev)])
    assert ops.spectral_layer_calls == before + 3, "the three encoder layers take the spectral form on a shared 2-D support"
    loss = utils.compute_regression_loss(y_true=y.to(dev), y_predicted=pred, standard_scaler=None, loss_fn="MAE")
    loss.backward()
    cfg = orc.DCRNNConfig(filter_type=filt, num_rnn_layers=3)
    po = {k: v.requires_grad_(True) for k, v in sc._params_of(model).items()}
    assert po["decoder.decoding_cells.2.dconv_gate.weight"] is po["decoder.decoding_cells.1.dconv_gate.weight"]
    torch.set_num_threads(16)
    pr = orc.next_time_pred_forward(po, cfg, x, y, [shared])
    lo = orc.regression_loss(y, pr, loss_fn="MAE")
    lo.backward()
    err_l = abs(loss.item() - lo.item()) / max(abs(lo.item()), 1e-12)
    print(f"ssl 3-layer distance graph: loss {loss.item():.7f} oracle {lo.item():.7f} (rel {err_l:.2e})")
    assert err_l < 1e-4
    for k, p in model.named_parameters():
        ref = po[k].grad
        err = (p.grad.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
        print(f"  d_{k}: {err:.2e}")
        assert err < 1e-4, f"{k}: {err:.2e}"
