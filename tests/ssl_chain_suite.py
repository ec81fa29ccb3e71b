"""Checks of the data side of the SSL step -- the sample is a PAIR (input clip, first seconds of the following clip), one coin and
one scale factor per sample on both halves, then the scaler on both (reference: data/dataloader_ssl.py:159-182,317-355).  As in
parity_suite.py the same functions run on the GPU library and on the emulator build of the same kernel sources
(tests/test_ssl_chain.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import assert_close_scaled, load, make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = 5.53, 0.65          # scaler of the step checks (the values check_augmented_step uses)


def oracle_pair(feats_x, feats_y, perm, log_scale, mean, std):
    """dataloader_ssl.py:317-336 on un-augmented features: feats_x (B,Tx,N,D) / feats_y (B,Ty,N,D) float64, perm (B,N) source
    channel per node (`EEG_seq_reflect[:, pair] = EEG_seq[:, swapped pair]`), log_scale (B,) = log(scale_factor) -> both halves
    reflected with the clip's perm, shifted by the clip's log scale, standardised (float64)."""
    perm, log_scale = np.asarray(perm), np.asarray(log_scale, dtype=np.float64)
    out = []
    for f in (feats_x, feats_y):
        fa = np.stack([f[i][:, perm[i], :] + log_scale[i] for i in range(f.shape[0])])
        out.append((fa - mean) / std)
    return out[0], out[1]


def check_oracle_pair_vs_reference():
    """the oracle chain above against the reference's own SSL loader (tests/golden/golden_ssl_pair_v1.npz, recorded by
    tests/golden/make_golden_ssl_pair.py): both outcomes of the coin, one scale factor on both halves, the scaler on both, the
    target cut to its first steps; the correlation graph of the sample is that of the un-reflected input clip either way."""
    from eeg_gnn_ssl_amd import utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_ssl_pair_v1.npz"))
    t_out = int(g["output_len"][0])
    mean, std = (float(v) for v in g["mean_std"])
    sp = utils.swap_permutation(19, [tuple(int(v) for v in p) for p in g["pairs"]]).numpy()
    assert sp.tolist() == utils.swap_permutation(19).tolist()
    fx, fy = g["clip_x"][None], g["clip_y"][None, :t_out]
    for tag, perm in (("reflected", sp), ("plain", np.arange(19))):
        x, y = oracle_pair(fx, fy, perm[None], np.log(g["scale"]), mean, std)
        np.testing.assert_allclose(x[0], g[f"{tag}/x"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(y[0], g[f"{tag}/y"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(utils.correlation_graph(g["clip_x"], top_k=3), g[f"{tag}/indiv_adj"], rtol=0, atol=2e-6)
    assert not np.array_equal(g["reflected/y"], g["plain/y"])
    assert np.array_equal(g["reflected/indiv_adj"], g["plain/indiv_adj"])


def _draws(b, g, n=19):
    """a perm / log_scale pair with both coin outcomes"""
    from eeg_gnn_ssl_amd import utils
    sp = utils.swap_permutation(n) if n == 19 else torch.arange(n - 1, -1, -1, dtype=torch.int32)
    flags = [(i % 2) == 1 for i in range(b)]
    perm = torch.stack([sp if f else torch.arange(n, dtype=torch.int32) for f in flags]).to(torch.int32)
    ls = torch.log(0.8 + 0.4 * torch.rand(b, generator=g)).float()
    return flags, perm, ls


def check_fft_features_pair(device):
    """`ops.fft_features_pair` (a) against the oracle chain -- `orc.fft_features` in float64 on the float32-rounded samples of both
    halves, both reflected with the clip's perm, + the clip's log scale, z-score -- at the 5e-6 absolute of
    `parity_suite.check_fft_features` for this comparison, and (b) bit-equal, output by output, to `ops.fft_features` on each half:
    the pair is a re-scheduling, not another transform.  3 x 19 x 5 = 285 and 3 x 19 x 3 = 171 windows: a partial last group of
    six in each half; the 200-sample kernel and the general one (window 40)."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(12)
    b, n, tx, ty = 3, 19, 5, 3
    mean, std = 0.5, 2.0
    for w in (200, 40):
        assert (b * n * tx) % 6 != 0 and (b * n * ty) % 6 != 0
        raw_x = 20.0 * torch.randn(b, n, tx * w, generator=g)
        raw_y = 20.0 * torch.randn(b, n, ty * w, generator=g)
        _, perm, ls = _draws(b, g)
        for pm, lg in ((perm, ls), (None, None)):
            pd, ld = (None, None) if pm is None else (pm.to(device), lg.to(device))
            fr, xs, ys = ops.fft_features_pair(raw_x.to(device), raw_y.to(device), window=w, mean=mean, std=std, perm=pd, log_scale=ld)
            assert fr.shape == xs.shape == (b, tx, n, w // 2) and ys.shape == (b, ty, n, w // 2)
            fx = np.stack([orc.fft_features(raw_x[i].numpy().astype(np.float64), window=w) for i in range(b)])
            fy = np.stack([orc.fft_features(raw_y[i].numpy().astype(np.float64), window=w) for i in range(b)])
            ex, ey = oracle_pair(fx, fy, np.tile(np.arange(n), (b, 1)) if pm is None else pm.numpy(),
                                 np.zeros(b) if lg is None else lg.numpy(), mean, std)
            for got, want, what in ((fr, fx, "feat_raw_x"), (xs, ex, "x_std"), (ys, ey, "y_std")):
                err = float(np.abs(got.cpu().numpy() - want).max())
                print(f"fft_features_pair W={w} augmented={pm is not None} {what}: max abs err {err:.3e}")
                assert err <= 5e-6, (w, what, err)
            fr1, xs1 = ops.fft_features(raw_x.to(device), window=w, mean=mean, std=std, perm=pd, log_scale=ld)
            _, ys1 = ops.fft_features(raw_y.to(device), window=w, mean=mean, std=std, perm=pd, log_scale=ld)
            assert torch.equal(fr, fr1) and torch.equal(xs, xs1) and torch.equal(ys, ys1), w


def torch_augment(x, perm, log_scale, feature_std):
    """the expression of TrainStep's supervised feature path"""
    idx = perm.to(torch.int64)[:, None, :, None].expand(-1, x.shape[1], -1, x.shape[3])
    return x.gather(2, idx) + (log_scale / feature_std)[:, None, None, None]


def check_augment_features(device):
    """`ops.augment_features` against the ATen expression of the supervised path applied to x and to y: bit for bit (one fp32 add
    per element: nothing to re-associate).  D = 100 and D = 36 (not a multiple of 32), another node count, clips with coin 0 and
    coin 1, x / y of different lengths, a clip size that is not a multiple of the launch's tile; inputs untouched."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(44)
    for (b, tx, ty, n, d) in ((4, 5, 2, 19, 100), (3, 2, 3, 19, 36), (2, 1, 1, 7, 4), (2, 13, 4, 19, 100)):
        x, y = torch.randn(b, tx, n, d, generator=g).to(device), torch.randn(b, ty, n, d, generator=g).to(device)
        flags, perm, ls = _draws(b, g, n)
        assert any(flags) and not all(flags)
        perm, ls = perm.to(device), ls.to(device)
        x0, y0 = x.clone(), y.clone()
        xa, ya = ops.augment_features(x, y, perm, ls, STD)
        assert torch.equal(x, x0) and torch.equal(y, y0)
        assert torch.equal(xa, torch_augment(x, perm, ls, STD)), (b, tx, n, d)
        assert torch.equal(ya, torch_augment(y, perm, ls, STD)), (b, ty, n, d)
        assert not torch.equal(xa[1], x[1] + ls[1] / STD)                     # the reflected clip did move rows
    # an entry outside 0..N-1 selects the node itself, as in the featurisation kernels
    ident = torch.arange(19, dtype=torch.int32, device=device).repeat(2, 1)
    ident_bad = ident.clone()
    ident_bad[0, 3], ident_bad[1, 7] = 99, -5
    a, c = ops.augment_features(x, y, ident, ls, STD), ops.augment_features(x, y, ident_bad, ls, STD)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def _oracle_step(params, cfg, x, y, sups, teacher):
    uniq, po = {}, {}
    for k, v in params.items():                                  # decoding_cells.l, l >= 2, alias decoding_cells.1: one leaf
        if id(v) not in uniq:
            uniq[id(v)] = v.clone().requires_grad_(True)
        po[k] = uniq[id(v)]
    pr = orc.next_time_pred_forward(po, cfg, x, y, sups, teacher_force_mask=teacher)
    lo = orc.regression_loss(y, pr, loss_fn="MAE")
    lo.backward()
    return lo, po


def _ssl_case(adj3d, graph, raw, b, t_in, t_out, curriculum, device, seed=57):
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    g = torch.Generator().manual_seed(seed)
    raw_x = 20.0 * torch.randn(b, 19, t_in * 200, generator=g)
    raw_y = 20.0 * torch.randn(b, 19, t_out * 200, generator=g)
    filt = "laplacian" if graph == "distance" else "dual_random_walk"
    # curriculum with the flags fixed: a decay constant so large that the sampling threshold (utils.py:385-390) is 1 - 1e-12 --
    # every step is teacher-forced, on the host (`random.random()`) and on the device (32-bit uniforms) alike
    cfg = orc.DCRNNConfig(filter_type=filt, use_curriculum_learning=curriculum, cl_decay_steps=10 ** 12 if curriculum else 3000)
    params = orc.init_params(cfg, "ssl", seed=3)
    args = make_args(cfg)
    args.use_curriculum_learning = curriculum
    model = DCRNNModel_nextTimePred(args, device=device)
    load(model, params, device)
    model.train()
    fx = np.stack([orc.fft_features(raw_x[i].numpy().astype(np.float64), window=200) for i in range(b)])      # (B, Tx, N, 100)
    fy = np.stack([orc.fft_features(raw_y[i].numpy().astype(np.float64), window=200) for i in range(b)])
    plain = utils.compute_supports(adj3d, filt)
    refl = utils.reflected_supports(adj3d, filt)
    kw = dict(raw_window=200, raw_mean=MEAN, raw_std=STD) if raw else dict(feature_std=STD)
    torch.manual_seed(1234)                                       # the seed of the step's augmentation generator
    st = TrainStep(model, task="ssl", data_augment=True, reflected_supports=refl if graph == "distance" else None, **kw)
    sup_in = [p_.unsqueeze(0).repeat(b, 1, 1).to(device) for p_ in plain] if graph == "distance" else None
    if raw:
        x_in, y_in = raw_x, raw_y
    else:
        x_in, y_in = (torch.from_numpy(((f - MEAN) / STD).astype(np.float32)) for f in (fx, fy))

    def oracle(flags, perm, ls, at=None):
        """the oracle chain for the draws of one step (at: other parameters than the initial ones) -> (loss, leaves with gradients)"""
        xa, ya = oracle_pair(fx, fy, perm.numpy(), ls.numpy().astype(np.float64), MEAN, STD)
        x, y = torch.from_numpy(xa.astype(np.float32)), torch.from_numpy(ya.astype(np.float32))
        if graph == "distance":
            sups = [torch.stack([(refl[k] if flags[i] else plain[k]) for i in range(b)]) for k in range(len(plain))]
        else:
            src = fx if raw else (fx - MEAN) / STD               # the graph of the un-augmented INPUT; the target plays no part
            per = [utils.compute_supports(utils.correlation_graph(src[i], top_k=3), filt) for i in range(b)]
            sups = [torch.stack([per[i][k] for i in range(b)]) for k in range(2)]
        return _oracle_step(params if at is None else at, cfg, x, y, sups, [True] * t_out if curriculum else None)

    return st, model, x_in.to(device), y_in.to(device), sup_in, oracle


def check_augmented_ssl_step(device, adj3d, graph="distance", raw=True, b=6, t_in=3, t_out=2, curriculum=False):
    """The SSL twin of `parity_suite.check_augmented_step`: TrainStep(task="ssl", data_augment=True) on
    `DCRNNModel_nextTimePred` with oracle parameters, two `forward_backward` calls; the draws are read back from
    `st.last_augmentation` and handed to the oracle chain (numpy FFT -> reflect x AND y -> + log scale -> z-score -> host graph
    builders -> `orc.next_time_pred_forward` -> `orc.regression_loss`): loss (2e-5 absolute) and every parameter gradient
    (`assert_close_scaled(tol=1e-4)`) agree; the draws of the two steps differ, both coin outcomes occurred, `eval()` draws
    nothing.  curriculum: every decoder step teacher-forced -- the augmented target is also what the decoder is fed.

    FAILS ON THE PARENT COMMIT: from features the target reaches decoder and loss un-reflected and un-scaled (the loss misses
    the oracle's by orders of magnitude more than 2e-5); from raw signals a raw target is not accepted at all."""
    st, model, x_in, y_in, sup_in, oracle = _ssl_case(adj3d, graph, raw, b, t_in, t_out, curriculum, device)
    draws = []
    for step in range(2):                                          # two steps: the generator advanced, the draws differ
        loss = st.forward_backward(x_in, y_in, None, sup_in)
        flags, perm, ls = (t.cpu() for t in st.last_augmentation)
        draws.append(flags.tolist() + ls.tolist())
        lo, po = oracle(flags, perm, ls)
        print(f"augmented ssl step {graph}/{'raw' if raw else 'features'} step {step}: loss {loss.item():.7f} oracle {lo.item():.7f}")
        assert abs(float(loss.item()) - float(lo.item())) < 2e-5, (float(loss.item()), float(lo.item()))
        for k, q in model.named_parameters():
            assert_close_scaled(q.grad.cpu().numpy(), po[k].grad.numpy(), f"augmented ssl step {graph}/d_{k}", tol=1e-4)
    assert draws[0] != draws[1]
    assert 0 < sum(draws[0][:b]) + sum(draws[1][:b]) < 2 * b       # both outcomes of the coin were exercised
    model.eval()                                                 # no augmentation outside training
    st.last_augmentation = None
    st.forward_backward(x_in, y_in, None, sup_in)
    assert st.last_augmentation is None


def _params_of(model):
    """the model's parameters as oracle leaves' sources (host copies; aliased entries stay one tensor)"""
    uniq, out = {}, {}
    for k, v in model.state_dict().items():
        if v.data_ptr() not in uniq:
            uniq[v.data_ptr()] = v.detach().cpu().clone()
        out[k] = uniq[v.data_ptr()]
    return out


def check_captured_ssl_step(device, adj3d, b=6, t_in=3, t_out=2):
    """`capture()` of the paired raw step (correlation graph, device curriculum) and three `replay_step()`s: every replay draws
    afresh (`last_augmentation` differs between replays) and its loss is the oracle's for the draws read back (2e-5 absolute, as
    in `check_augmented_ssl_step`), on the parameters that replay started from (a replay ends with the optimiser's update)."""
    st, model, x_in, y_in, sup_in, oracle = _ssl_case(adj3d, "correlation", True, b, t_in, t_out, True, device)
    st.capture(x_in, y_in, None, sup_in)
    assert st.device_curriculum is True
    seen = []
    for r in range(3):
        before = _params_of(model)
        loss = float(st.replay_step().item())
        flags, perm, ls = (t.cpu().clone() for t in st.last_augmentation)
        seen.append(flags.tolist() + ls.tolist())
        lo, _ = oracle(flags, perm, ls, before)
        print(f"captured ssl step replay {r}: loss {loss:.7f} oracle {lo.item():.7f} flags {flags.tolist()}")
        assert abs(loss - float(lo.item())) < 2e-5, (r, loss, float(lo.item()))
    assert seen[0] != seen[1] and seen[1] != seen[2] and seen[0] != seen[2]
    assert st.samples_seen == 3 * b and st.step_count == 3


def check_refusals(device):
    """operands that do not fit are refused loudly, at the operator and at the C ABI (`eeg_dcrnn_last_error` names the cause)"""
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, _lib, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    z = lambda *s: torch.zeros(*s, device=device)     # noqa: E731
    n = 19
    ident = torch.arange(n, dtype=torch.int32, device=device).repeat(2, 1)
    for what, call, msg in (
            ("raw target of a broken window", lambda: ops.fft_features_pair(z(2, n, 400), z(2, n, 250), window=200), "raw target signals must be"),
            ("raw target of another batch", lambda: ops.fft_features_pair(z(2, n, 400), z(3, n, 200), window=200), "raw target signals must be"),
            ("raw input 2-D", lambda: ops.fft_features_pair(z(n, 400), z(2, n, 200), window=200), "raw input signals must be"),
            ("pair: perm of another shape", lambda: ops.fft_features_pair(z(2, n, 400), z(2, n, 200), window=200, perm=ident[:1]), "perm has shape"),
            ("pair: log_scale of another batch", lambda: ops.fft_features_pair(z(2, n, 400), z(2, n, 200), window=200, log_scale=z(3)), "log_scale has 3"),
            ("augment: perm of another shape", lambda: ops.augment_features(z(2, 3, n, 8), z(2, 2, n, 8), ident[:1], z(2), 1.0), "perm has shape"),
            ("augment: log_scale of another batch", lambda: ops.augment_features(z(2, 3, n, 8), z(2, 2, n, 8), ident, z(5), 1.0), "log_scale has 5"),
            ("augment: target of another width", lambda: ops.augment_features(z(2, 3, n, 8), z(2, 2, n, 12), ident, z(2), 1.0), "target features must be"),
            ("augment: D not a multiple of 4", lambda: ops.augment_features(z(2, 3, n, 6), z(2, 2, n, 6), ident, z(2), 1.0), "feature dim=6"),
            ("augment: zero std", lambda: ops.augment_features(z(2, 3, n, 8), z(2, 2, n, 8), ident, z(2), 0.0), "feature_std"),
    ):
        with pytest.raises(RuntimeError, match=msg):
            call()
            pytest.fail(f"{what}: accepted")
    if device != "cpu":                   # a HOST perm that is not a permutation never reaches the kernel (feat_raw_x is written at the source slot)
        bad = torch.arange(n, dtype=torch.int32).repeat(2, 1)
        bad[0, 3] = 4
        with pytest.raises(RuntimeError, match="permutation"):
            ops.fft_features_pair(z(2, n, 400), z(2, n, 200), window=200, perm=bad)
    # TrainStep: a raw SSL target that is not a whole number of windows / not 3-D names the expected shape
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk")
    model = DCRNNModel_nextTimePred(make_args(cfg), device=device).to(device)
    st = TrainStep(model, task="ssl", raw_window=200)
    for bad_y in (z(2, n, 250), z(2, 2, n, 100)):
        with pytest.raises(ValueError, match=r"RAW target \(B, num_nodes, Ty\*200\)"):
            st.forward_backward(z(2, n, 400), bad_y, None, None)
    # C ABI: null outputs, degenerate sizes
    lib = _lib.get_lib()
    x, y, out = z(2, n, 400), z(2, n, 200), z(2, 2, n, 100)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    pair = lambda *a: lib.query("eeg_dcrnn_fft_features_pair", *a)     # noqa: E731
    aug = lambda *a: lib.query("eeg_dcrnn_augment_features", *a)     # noqa: E731
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 1.0, None, p(out), None, None), "fft_features_pair: null output")
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 1.0, None, None, p(out), None), "fft_features_pair: null output")
    refused(pair(p(x), None, 2, n, 2, 1, 200, None, None, 0.0, 1.0, None, p(out), p(out), None), "fft_features_pair: null input")
    refused(pair(p(x), p(y), 2, n, 2, 0, 200, None, None, 0.0, 1.0, None, p(out), p(out), None), "fft_features_pair: empty input")
    refused(pair(p(x), p(y), 2, n, 2, 1, 202, None, None, 0.0, 1.0, None, p(out), p(out), None), "window=202 unsupported")
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 0.0, None, p(out), p(out), None), "std must be non-zero")
    fx, fy, ox, oy, sh = z(2, 2, n, 8), z(2, 1, n, 8), z(2, 2, n, 8), z(2, 1, n, 8), z(2)
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sh), None, p(oy), None), "augment_features: null output")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sh), p(ox), None, None), "augment_features: null output")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, None, p(sh), p(ox), p(oy), None), "augment_features: null input / perm / shift")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sh), p(fx), p(oy), None), "in-place")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 6, p(ident), p(sh), p(ox), p(oy), None), "feature dim=6 unsupported")
    refused(aug(p(fx), p(fy), 0, 2, 1, n, 8, p(ident), p(sh), p(ox), p(oy), None), "augment_features: empty input")
