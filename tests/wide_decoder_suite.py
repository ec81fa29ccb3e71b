"""Checks of the persistent decoder kernels at outputs wider than 128 (time-domain SSL: input_dim = output_dim = 200): which shapes
they cover, decoder and model against the oracle under the decoder's own criteria (parity_suite.check_decoder_vs_oracle,
parity_suite.check_ssl_device_curriculum), that the persistent kernels are what ran, graph replay under curriculum learning, and
run-to-run determinism.  Run by tests/test_wide_decoder.py on the emulator build of the kernel sources and on the MI355X library."""
import numpy as np
import torch

import cases
import parity_suite as ps
from oracle import dcrnn_oracle as orc

# (t, b, n, h, dout, m, layers) -> the persistent kernels cover it
CAPABILITY = [
    ((12, 512, 19, 64, 200, 5, 2), True),      # correlation graph, two layers: 162 112 B of LDS in the forward, the edge
    ((12, 8, 19, 64, 200, 3, 3), True),        # the README's SSL recipe on the distance graph
    ((12, 8, 19, 64, 256, 3, 2), True),        # sixteen output tiles
    ((12, 8, 19, 64, 200, 5, 3), False),       # LDS
    ((12, 8, 19, 64, 256, 5, 2), False),       # LDS
    ((12, 8, 19, 64, 200, 7, 1), False),       # LDS
    ((12, 8, 19, 64, 136, 3, 2), False),       # Dout / 4 = 34: no weight-group size of the projection transpose divides it
    ((12, 8, 19, 64, 260, 3, 2), False),       # wider than the input-gradient tiles of a wave reach
]

# filt, dout, layers, t_out, b, ratio, n, order, seed (the seed only picks the host coin flips of `ratio`: mixed flags required)
WIDE_SHAPES = {
    "m5_autoregressive_200": ("dual_random_walk", 200, 2, 3, 2, None, 19, 2, 3),   # every step takes the wide tail; M = 5 at the LDS edge
    "shared_cell_host_flags_200": ("laplacian", 200, 3, 4, 2, 0.5, 19, 2, 3),      # pairs with and without a wanted dX; shared cell
    "device_flags_200": ("dual_random_walk", 200, 2, 4, 3, "device", 19, 2, 3),    # flags from device memory
    "nine_tiles_20_nodes": ("laplacian", 144, 2, 3, 2, None, 20, 2, 3),            # only wave 0 has a third tile; remainder tile full
    "eleven_tiles_m2": ("laplacian", 176, 2, 3, 2, 0.5, 19, 1, 3),                 # three waves with a one-tile tail; M = 2
    "sixteen_tiles_256": ("laplacian", 256, 2, 2, 2, None, 19, 2, 3),              # every wave a two-tile tail; DT = 4
}
MANY_CLIPS = ("dual_random_walk", 200, 2, 2, 300, None, 19, 2, 3)                  # more clips than workgroups (GPU only)


def hops(filt, order):
    return (2 if filt == "dual_random_walk" else 1) * order + 1


def check_capability_table():
    from eeg_gnn_ssl_amd import ops
    for dims, want in CAPABILITY:
        assert ops.decoder_is_persistent(*dims) is want, (dims, want)
    # narrower shapes answer as before
    assert ops.decoder_is_persistent(12, 512, 19, 64, 100, 5, 2) and ops.decoder_is_persistent(12, 8, 19, 64, 100, 5, 3)
    assert not ops.decoder_is_persistent(12, 8, 19, 64, 36, 3, 2) and not ops.decoder_is_persistent(4, 2, 19, 32, 20, 3, 2)


def check_wide_shape(device, adj3d, shape):
    from eeg_gnn_ssl_amd import ops
    filt, dout, layers, t_out, b, ratio, n, order, seed = shape
    assert ops.decoder_is_persistent(t_out, b, n, 64, dout, hops(filt, order), layers), shape
    ps.check_decoder_vs_oracle(device, filt, dout, 64, layers, t_out, b, adj3d, seed=seed, ratio=ratio, n=n, order=order)


def _decoder_run(device, adj3d, shape):
    """one forward + backward of DCGRUDecoder on fixed random inputs -> (outputs, dh0, parameter gradients)"""
    from eeg_gnn_ssl_amd import DCGRUDecoder
    filt, dout, layers, t_out, b, _, n, order, seed = shape
    g = torch.Generator().manual_seed(seed)
    cfg = orc.DCRNNConfig(filter_type=filt, input_dim=dout, output_dim=dout, rnn_units=64, num_rnn_layers=layers, num_nodes=n,
                          max_diffusion_step=order)
    params = {k[len("decoder."):]: v for k, v in orc.init_params(cfg, "ssl", seed=seed).items() if k.startswith("decoder.")}
    dec = DCGRUDecoder(input_dim=dout, max_diffusion_step=order, num_nodes=n, hid_dim=64, output_dim=dout, num_rnn_layers=layers,
                       dcgru_activation="tanh", filter_type=filt)
    ps.load(dec, params, device)
    dec.train()
    sup = [s.to(device) for s in cases.supports_for(filt, adj3d, b)]
    targets = torch.randn(t_out, b, n, dout, generator=g).to(device)
    h0 = (0.5 * torch.randn(layers, b, n * 64, generator=g)).to(device)
    wout = torch.randn(t_out, b, n * dout, generator=g).to(device)

    def run():
        dec.zero_grad()
        h0d = h0.clone().requires_grad_(True)
        out = dec(targets, h0d, sup, teacher_forcing_ratio=None)
        (out * wout).sum().backward()
        return [out.detach().clone(), h0d.grad.clone()] + [p.grad.clone() for p in dec.parameters()]
    return run


def check_persistent_kernels_ran(device, adj3d):
    """the event recorder around one forward + backward at the first wide shape: one persistent forward, one persistent backward, and
    none of the per-step decoder launches (x-part / projection / input-gradient GEMMs, T = 1 recurrent launches, node mixes)"""
    run = _decoder_run(device, adj3d, WIDE_SHAPES["m5_autoregressive_200"])
    run()                                                   # (first call: allocations)
    torch.cuda.synchronize()
    counts = {role: sum(by_symbol.values()) for role, by_symbol in ps.kernels_run(run).items()}
    assert counts.get("dec_fwd_persist") == 1 and counts.get("dec_bwd_persist") == 1, counts
    per_step = [r for r in counts if r.startswith(("dec_gemm_nn", "dec_seq_", "dec_diffuse_", "dec_gemm_dx"))]
    assert not per_step, counts


def check_determinism(device, adj3d, repeats=50):
    run = _decoder_run(device, adj3d, WIDE_SHAPES["m5_autoregressive_200"])
    first = run()
    for _ in range(repeats - 1):
        for a, b in zip(first, run()):
            assert torch.equal(a, b)


CL_DECAY, CL_SEEN0, CL_INCREMENT, CL_SEED, CL_OFFSET = 50.0, 196, 24, 20240917, 3      # ratio ~ 0.5 at 196 samples seen


def check_model_device_curriculum(device, adj3d, dropout=0.5, reps=3):
    """parity_suite.check_ssl_device_curriculum at input_dim = output_dim = 200 on random inputs (b = 3, t_in = 2, t_out = 4): the
    flags the kernels read are re-derived from the generator pair and handed to the oracle; predictions under `assert_close`, every
    gradient under `assert_close_scaled`; mixed flags occur within the repetitions (seed and decay checked on the host below)."""
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, ops, utils
    b, t_in, t_out, n, h, dim = 3, 2, 4, 19, 64, 200
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=dim, output_dim=dim)
    g = torch.Generator().manual_seed(11)
    params = orc.init_params(cfg, "ssl", seed=5)
    x, y = torch.randn(b, t_in, n, dim, generator=g), torch.randn(b, t_out, n, dim, generator=g)
    sup = cases.supports_for(cfg.filter_type, adj3d, b)
    args = ps._dropout_args(cfg, dropout)
    args.use_curriculum_learning = True
    args.cl_decay_steps = int(CL_DECAY)
    model = DCRNNModel_nextTimePred(args, device=device)
    ps.load(model, params, device)
    model.train()
    assert ops.decoder_is_persistent(t_out, b, n, h, dim, 5, cfg.num_rnn_layers)
    xd, yd, supd = x.to(device), y.to(device), [s.to(device) for s in sup]
    seen = torch.tensor([CL_SEEN0], dtype=torch.int64, device=device)
    model.batches_seen_increment = CL_INCREMENT
    model.decoder.set_dropout_seed(CL_SEED, CL_OFFSET)
    drawn = []
    for _ in range(reps):
        seed, off = model.decoder.dropout_rng_state()
        n_seen = int(seen.item())
        flags = ps.expected_teacher_flags(seed, off, n_seen, CL_DECAY, t_out)
        drawn.append(flags.tolist())
        model.zero_grad()
        pred = model(xd, yd, supd, batches_seen=seen)
        assert int(seen.item()) == n_seen + CL_INCREMENT
        masks = None
        if dropout > 0:
            groups = t_out * b * n * h // 4
            used = torch.tensor([seed, off + (t_out + 3) // 4], dtype=torch.int64, device=device)
            masks = ops.dropout_mask(used, 4 * groups, dropout).view(t_out, b, n, h).cpu()
            assert model.decoder.dropout_rng_state() == (seed, off + (t_out + 3) // 4 + groups)
        else:
            assert model.decoder.dropout_rng_state() == (seed, off + (t_out + 3) // 4)
        loss = utils.compute_regression_loss(y_true=yd, y_predicted=pred, standard_scaler=utils.StandardScaler(cases.SSL_MEAN, cases.SSL_STD),
                                             loss_fn="MAE")
        loss.backward()
        uniq, po = {}, {}
        for k, v in params.items():
            if id(v) not in uniq:
                uniq[id(v)] = v.clone().requires_grad_(True)
            po[k] = uniq[id(v)]
        pro = orc.next_time_pred_forward(po, cfg, x, y, sup, teacher_force_mask=[bool(v) for v in flags], dropout_masks=masks)
        orc.regression_loss(y, pro, cases.SSL_MEAN, cases.SSL_STD, loss_fn="MAE").backward()
        ps.assert_close(pred.detach().cpu().numpy(), pro.detach().numpy(), f"device curriculum at 200 wide: pred (flags {flags.tolist()})")
        for k, q in model.named_parameters():
            ps.assert_close_scaled(q.grad.cpu().numpy(), po[k].grad.numpy(), f"device curriculum at 200 wide: d_{k}")
    assert len({tuple(f) for f in drawn}) > 1 and any(0 < sum(f[:-1]) < t_out - 1 for f in drawn), drawn


def check_curriculum_graph_replay(device, steps=6):
    """`TrainStep(use_fft=False)` on ready 200-sample windows with curriculum learning: eager steps against capture + replays from
    the same seeds -- flags on the device, losses pairwise equal and all different, parameters bit-equal, counters equal."""
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred
    from eeg_gnn_ssl_amd.train_step import TrainStep
    g = torch.Generator().manual_seed(9)
    b, t_in, t_out, dim = 3, 2, 5, 200
    x = torch.randn(b, t_in, 19, dim, generator=g).to(device)
    y = torch.randn(b, t_out, 19, dim, generator=g).to(device)
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=dim, output_dim=dim)
    args = ps._dropout_args(cfg, 0.5)
    args.use_curriculum_learning = True
    args.cl_decay_steps = 12                   # ratio = 12 / (12 + exp(n / 12)): ~0.5 after ~30 samples
    finals, losses, seen = [], [], []
    for graphed in (False, True):
        torch.manual_seed(1)
        model = DCRNNModel_nextTimePred(args, device=device).to(device).train()
        st = TrainStep(model, task="ssl", lr=1e-3, use_fft=False, feature_mean=cases.SSL_MEAN, feature_std=cases.SSL_STD)
        model.decoder.set_dropout_seed(777, 0)
        if graphed:
            st.capture(x, y, None, None)       # supports built on the device inside the step
            assert st.samples_seen == 0 and int(st.samples_seen_dev.item()) == 0
            model.decoder.set_dropout_seed(777, 0)
        ls = [float((st.replay_step() if graphed else st.step(x, y, None, None)).item()) for _ in range(steps)]
        torch.cuda.synchronize()
        assert st.device_curriculum is True
        finals.append(st.fp.flat.detach().clone())
        losses.append(ls)
        seen.append((st.samples_seen, int(st.samples_seen_dev.item()), model.decoder.dropout_rng_state()))
    assert seen[0] == seen[1] and seen[0][0] == seen[0][1] == steps * b
    assert len(set(losses[1])) == steps, losses
    assert losses[0] == losses[1], losses
    assert torch.equal(finals[0], finals[1])
    assert np.isfinite(losses[0]).all()
