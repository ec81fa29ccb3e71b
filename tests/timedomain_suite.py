"""Checks of the time-domain input mode (the reference without --use_fft: a step of a clip is its 200 samples, `_random_scale`
multiplies; data/dataloader_detection.py:25-85,233-307, data/dataloader_ssl.py:159-182,317-355): windowing + augmentation + scaler
from raw signals, the same augmentation on ready windows, the correlation graph of wide channel rows, and `TrainStep(use_fft=False)`.
As in ssl_chain_suite.py the same functions run on the GPU library and on the emulator build of the same kernel sources
(tests/test_timedomain.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import assert_close_scaled, load, make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = 0.37, 21.3           # scaler of the operator and step checks (neither is an fp32 number)
EPS = 2.0 ** -24                  # half an ulp of 1: the relative error of one fp32 rounding


# ---- the oracle chain (numpy, float64) -------------------------------------------------------------------------------------------
def oracle_windows(raw, window, perm=None, scale=None, mean=0.0, std=1.0):
    """dataloader_detection.py:25-85 (`computeSliceMatrix(is_fft=False)`), :233-256 and utils.py:393-428 in closed form:
    raw (B, N, T*W) float64 -> (B, T, N, W) = (raw[b, perm[b][n], t*W ..] * scale[b] - mean) / std"""
    raw = np.asarray(raw, dtype=np.float64)
    b, n, total = raw.shape
    clip = raw.reshape(b, n, total // window, window).transpose(0, 2, 1, 3)
    if perm is not None:
        clip = np.stack([clip[i][:, np.asarray(perm[i]), :] for i in range(b)])
    if scale is not None:
        clip = clip * np.asarray(scale, dtype=np.float64)[:, None, None, None]
    return (clip - mean) / std


def golden_signals(seed, length, n=19):
    """the seeded channel rows of tests/golden/make_golden_timedomain.py (`signals` there)"""
    rs = np.random.RandomState(100 + seed)
    mix, src, noise = rs.standard_normal((n, 5)), rs.standard_normal((5, length)), rs.standard_normal((n, length))
    return 30.0 * (mix @ src + 0.7 * noise)


def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_timedomain_v1.npz"))
    t_len, n, w, t_out, top_k = (int(v) for v in g["shape"])
    return g, t_len, n, w, t_out, top_k


def check_chain_vs_reference():
    """the numpy chain above against the reference's own loaders in time-domain mode (golden_timedomain_v1.npz, recorded by
    tests/golden/make_golden_timedomain.py): both outcomes of the coin, the factor the detection loader drew, the SSL loader with
    the same draws on input and target, the scaler on both, the target cut to its first steps (1e-12); the correlation graph is that
    of the un-augmented clip = of the raw channel rows, on either layout (2e-6)."""
    from eeg_gnn_ssl_amd import utils
    g, t_len, n, w, t_out, top_k = _golden()
    mean, std = (float(v) for v in g["mean_std"])
    sp = utils.swap_permutation(n).numpy()
    for tag, perm in (("reflected", sp), ("plain", np.arange(n))):
        raw = golden_signals(int(g[f"{tag}/seed"][0]), 2 * t_len * w)
        rx, ry = raw[None, :, :t_len * w], raw[None, :, t_len * w:]
        x = oracle_windows(rx, w, perm[None], g[f"{tag}/scale"], mean, std)
        y = oracle_windows(ry, w, perm[None], g[f"{tag}/scale"], mean, std)[:, :t_out]
        np.testing.assert_allclose(x[0], g[f"{tag}/x"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(y[0], g[f"{tag}/y"], rtol=0, atol=1e-12)
        clip = oracle_windows(rx, w)[0]                                                  # (T, N, W), un-augmented
        np.testing.assert_allclose(utils.correlation_graph(clip, top_k=top_k), g[f"{tag}/indiv_adj"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(utils.correlation_graph(rx[0][None], top_k=top_k), g[f"{tag}/indiv_adj"], rtol=0, atol=2e-6)
    assert not np.array_equal(g["reflected/x"], g["plain/x"])


def _draws(b, g, n=19):
    """a perm / scale pair with both coin outcomes"""
    from eeg_gnn_ssl_amd import utils
    sp = utils.swap_permutation(n) if n == 19 else torch.arange(n - 1, -1, -1, dtype=torch.int32)
    flags = [(i % 2) == 1 for i in range(b)]
    perm = torch.stack([sp if f else torch.arange(n, dtype=torch.int32) for f in flags]).to(torch.int32)
    scale = (0.8 + 0.4 * torch.rand(b, generator=g)).float()
    return flags, perm, scale


def _signals(g, b, n, length, amp=20.0):
    """(B, N, length) float32 channel rows: shared sources + noise (correlations of every size: no near-ties at the top-k cut)"""
    mix, src = torch.randn(b, n, 5, generator=g), torch.randn(b, 5, length, generator=g)
    return (amp * (mix @ src + 0.7 * torch.randn(b, n, length, generator=g))).float()


def _window_bound(raw, window, perm, scale, mean, std):
    """4 * 2^-24 * (|v*s| + |mean|) / |std| per element: one rounding each for product, difference and quotient, plus one spare"""
    mag = np.abs(oracle_windows(raw, window, perm, scale, 0.0, 1.0))
    return 4.0 * EPS * (mag + abs(mean)) / abs(std)


# ---- operators -------------------------------------------------------------------------------------------------------------------
def check_window_features(device):
    """`ops.window_features` / `ops.window_features_pair` against the float64 chain on the fp32-rounded samples and the fp32 scale
    actually passed, element by element within `_window_bound` (no absolute tolerance); W = 200 and W = 40, with and without draws;
    3 * 19 * (5 + 3) * W / 4 pieces per launch: ragged last groups of the 1024-piece stretches.  The pair equals the single-buffer
    operator on each half bit for bit."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(12)
    b, n, tx, ty = 3, 19, 5, 3
    for w in (200, 40):
        assert ((tx + ty) * n * (w // 4)) % 1024 != 0 and (tx * n * (w // 4)) % 1024 != 0
        raw_x, raw_y = _signals(g, b, n, tx * w), _signals(g, b, n, ty * w)
        _, perm, scale = _draws(b, g)
        for pm, sc in ((perm, scale), (None, None), (perm, None), (None, scale)):
            pd = None if pm is None else pm.to(device)
            sd = None if sc is None else sc.to(device)
            xs, ys = ops.window_features_pair(raw_x.to(device), raw_y.to(device), w, MEAN, STD, perm=pd, scale=sd)
            assert xs.shape == (b, tx, n, w) and ys.shape == (b, ty, n, w)
            pn = None if pm is None else pm.numpy()
            sn = None if sc is None else sc.numpy().astype(np.float64)
            for got, src, what in ((xs, raw_x, "x_std"), (ys, raw_y, "y_std")):
                want = oracle_windows(src.numpy(), w, pn, sn, MEAN, STD)
                ratio = float((np.abs(got.cpu().numpy().astype(np.float64) - want) / _window_bound(src.numpy(), w, pn, sn, MEAN, STD)).max())
                print(f"window_features_pair W={w} perm={pm is not None} scale={sc is not None} {what}: worst error / bound {ratio:.3f}")
                assert ratio <= 1.0, (w, what, ratio)
            xs1 = ops.window_features(raw_x.to(device), w, MEAN, STD, perm=pd, scale=sd)
            ys1 = ops.window_features(raw_y.to(device), w, MEAN, STD, perm=pd, scale=sd)
            assert torch.equal(xs, xs1) and torch.equal(ys, ys1), w
        assert not torch.equal(xs[1], ops.window_features(raw_x.to(device), w, MEAN, STD)[1])      # clip 1 was reflected and scaled


def torch_augment_windows(x, perm, a, c):
    """the ATen expression of the augmentation behind the scaler"""
    idx = perm.to(torch.int64)[:, None, :, None].expand(-1, x.shape[1], -1, x.shape[3])
    return x.gather(2, idx) * a[:, None, None, None] + c[:, None, None, None]


def _ulp_distance(got, want):
    """|got - want| in units of the spacing of fp32 numbers at `want`"""
    want = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def check_augment_windows(device):
    """`ops.augment_windows` against the ATen expression `x.gather(2, idx) * a + c` on x and on y within 2 ulp of the result (FMA
    contraction may differ), and against the raw route -- `ops.window_features` of the same signals with the same draws -- within
    the bound of `check_window_features`.  D = 200 and D = 36, another node count, clips with both coin outcomes, y absent.
    Measured (emulator and MI355X alike: both routes use the same roundings in both builds): 0.00 ulp from the ATen expression
    everywhere; against the raw route at most 0.9999 of the bound -- two fp32 results, each within ~0.7 of it, that are two ulps
    apart for values just above a power of two, where that bound is two ulps wide."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(44)
    for (b, tx, ty, n, d) in ((4, 5, 2, 19, 200), (3, 2, 3, 19, 36), (2, 1, 1, 7, 4), (2, 7, 0, 19, 200)):
        raw_x, raw_y = _signals(g, b, n, tx * d), _signals(g, b, n, max(ty, 1) * d)
        flags, perm, scale = _draws(b, g, n)
        assert any(flags) and not all(flags)
        x = torch.from_numpy(oracle_windows(raw_x.numpy(), d, None, None, MEAN, STD).astype(np.float32)).to(device)
        y = torch.from_numpy(oracle_windows(raw_y.numpy(), d, None, None, MEAN, STD).astype(np.float32)).to(device) if ty else None
        perm_d, scale_d = perm.to(device), scale.to(device)
        x0 = x.clone()
        xa, ya = ops.augment_windows(x, y, perm_d, scale_d, MEAN, STD)
        assert torch.equal(x, x0) and (ya is None) == (y is None)
        c = (scale_d - 1.0) * (MEAN / STD)
        for got, src, rw in ((xa, x, raw_x), (ya, y, raw_y)):
            if src is None:
                continue
            want = torch_augment_windows(src, perm_d, scale_d, c)
            ulps = float(_ulp_distance(got.cpu().numpy(), want.cpu().numpy()).max())
            print(f"augment_windows B={b} N={n} D={d}: worst distance from the ATen expression {ulps:.2f} ulp")
            assert ulps <= 2.0, (b, n, d, ulps)
            # the raw route: the same signals, windowed, augmented and standardised in one pass
            direct = ops.window_features(rw.to(device), d, MEAN, STD, perm=perm_d, scale=scale_d).cpu().numpy().astype(np.float64)
            bound = _window_bound(rw.numpy(), d, perm.numpy(), scale.numpy().astype(np.float64), MEAN, STD)
            ratio = float((np.abs(got.cpu().numpy().astype(np.float64) - direct) / bound).max())
            print(f"augment_windows B={b} N={n} D={d}: worst distance from the raw route / bound {ratio:.3f}")
            assert ratio <= 1.0, (b, n, d, ratio)
        assert not torch.equal(xa[1], x[1] * scale_d[1] + c[1])                      # the reflected clip did move rows
    ident = torch.arange(19, dtype=torch.int32, device=device).repeat(2, 1)         # an entry outside 0..N-1 selects the node itself
    bad = ident.clone()
    bad[0, 3], bad[1, 7] = 99, -5
    assert torch.equal(ops.augment_windows(x, None, ident, scale_d, MEAN, STD)[0], ops.augment_windows(x, None, bad, scale_d, MEAN, STD)[0])


def _graph_errors(adj, s1, s2, rows, top_k):
    """(pattern equal, worst absolute error) of one clip's outputs against the float64 oracle on its channel rows (N, L)"""
    a_ref = orc.correlation_adjacency(rows[None].astype(np.float64), top_k=top_k)      # a clip of one step: (1, N, L)
    sup = [orc.random_walk(a_ref).T, orc.random_walk(a_ref.T).T]
    same = bool(((adj != 0) == (a_ref != 0)).all())
    return same, max(float(np.abs(adj - a_ref).max()), float(np.abs(s1 - sup[0]).max()), float(np.abs(s2 - sup[1]).max()))


def check_corr_graph_rows(device, repeats=3):
    """The Gram of wide channel rows -> supports: (a) the golden of the reference's `_get_indiv_graphs` in time-domain mode (2e-6);
    (b) the oracle on random rows with a silent channel and a strongly correlated pair, L in {8, 600, 2400, 7680}, N in {4, 12, 19,
    32}: pattern equality and 5e-6 absolute, the criterion of `parity_suite.check_correlation_supports`; (c) the window layout
    (B, T, N, 200), the raw layout and the oracle against each other; (d) `repeats` runs bit-identical; (e) `ops.correlation_supports`
    at D = 100 still IS the existing kernel, bit for bit, and at D = 200 takes the new one."""
    from eeg_gnn_ssl_amd import ops
    g, t_len, n, w, _, top_k = _golden()
    for tag in ("reflected", "plain"):
        raw = torch.from_numpy(golden_signals(int(g[f"{tag}/seed"][0]), 2 * t_len * w)[None, :, :t_len * w].astype(np.float32)).to(device)
        _, adj = ops.correlation_supports_raw(raw, top_k=top_k, return_adj=True)
        err = float(np.abs(adj[0].cpu().numpy() - g[f"{tag}/indiv_adj"]).max())
        print(f"corr_graph_rows vs the reference's graph ({tag}): {err:.2e}")
        assert err <= 2e-6
    gen = torch.Generator().manual_seed(9)
    for (b, n, length, k) in ((3, 4, 8, 2), (5, 19, 600, 3), (2, 12, 2400, 4), (2, 32, 7680, 31), (3, 19, 7680, 3), (2, 32, 600, 5),
                              (300, 19, 600, 3)):
        rows = torch.randn(b, n, length, generator=gen)
        rows[0, min(3, n - 1), :] = 0.0                        # a silent electrode: zero norm -> raw (zero) correlation
        rows[-1] = rows[-1] * 0.5 + rows[-1, :1, :]            # strongly correlated channels
        (s1, s2), adj = ops.correlation_supports_raw(rows.to(device), top_k=k, return_adj=True)
        for i in range(b if b < 10 else 4):
            same, err = _graph_errors(adj[i].cpu().numpy(), s1[i].cpu().numpy(), s2[i].cpu().numpy(), rows[i].numpy(), k)
            assert same, (b, n, length, i)
            assert err <= 5e-6, (b, n, length, i, err)
    # (c) layouts: the same clips as raw rows (B, N, T*200) and as windows (B, T, N, 200)
    b, n, t_len = 3, 19, 7
    raw = _signals(gen, b, n, t_len * 200)
    win = torch.from_numpy(oracle_windows(raw.numpy(), 200).astype(np.float32))
    assert torch.equal(win[1, 2, 5], raw[1, 5, 400:600])
    (r1, r2), radj = ops.correlation_supports_raw(raw.to(device), return_adj=True)
    (w1, w2), wadj = ops.correlation_supports(win.to(device), return_adj=True)             # D = 200 > 128: routed to the new kernel
    for i in range(b):
        for adj, s1, s2 in ((radj, r1, r2), (wadj, w1, w2)):
            same, err = _graph_errors(adj[i].cpu().numpy(), s1[i].cpu().numpy(), s2[i].cpu().numpy(), raw[i].numpy(), 3)
            assert same and err <= 5e-6, (i, err)
    assert float((radj - wadj).abs().max()) <= 1e-5 and torch.equal(radj != 0, wadj != 0)
    # (d) fixed-order sums: bit-reproducible
    rd = raw.to(device)
    for _ in range(repeats):
        (q1, q2), qadj = ops.correlation_supports_raw(rd, return_adj=True)
        assert torch.equal(qadj, radj) and torch.equal(q1, r1) and torch.equal(q2, r2)
    # (e) routing
    feats = torch.randn(4, 6, 19, 100, generator=gen).to(device)
    (f1, f2), fadj = ops.correlation_supports(feats, return_adj=True)
    padj, p1, p2 = torch.ops.eeg_dcrnn.corr_graph(feats, 3)
    assert torch.equal(fadj, padj) and torch.equal(f1, p1) and torch.equal(f2, p2)


def check_corr_graph_rows_long(device, b=2):
    """Rows of 12 000 samples (60 s at 200 Hz), a length the existing graph test never reaches: the new kernel's error against the
    float64 oracle may not exceed max(5e-6, 2 x the error of the existing kernel on the same values laid out as (B, 120, N, 100));
    the factor 2 because the two kernels sum in different orders.  Both errors are printed (MI355X, B = 8: rows kernel 1.8e-7,
    existing kernel 2.4e-7; emulator, B = 2: 1.2e-7 both)."""
    from eeg_gnn_ssl_amd import ops
    gen = torch.Generator().manual_seed(31)
    n, length = 19, 12000
    raw = _signals(gen, b, n, length)
    steps = raw.reshape(b, n, 120, 100).permute(0, 2, 1, 3).contiguous()                  # the same rows, as 120 steps of 100
    (r1, r2), radj = ops.correlation_supports_raw(raw.to(device), return_adj=True)
    oadj, o1, o2 = torch.ops.eeg_dcrnn.corr_graph(steps.to(device), 3)
    err_new = err_old = 0.0
    for i in range(b):
        same_n, e_n = _graph_errors(radj[i].cpu().numpy(), r1[i].cpu().numpy(), r2[i].cpu().numpy(), raw[i].numpy(), 3)
        same_o, e_o = _graph_errors(oadj[i].cpu().numpy(), o1[i].cpu().numpy(), o2[i].cpu().numpy(), raw[i].numpy(), 3)
        assert same_n and same_o, i
        err_new, err_old = max(err_new, e_n), max(err_old, e_o)
    print(f"corr graph at L = 12000: rows kernel {err_new:.2e}, existing kernel on (B,120,N,100) {err_old:.2e}")
    assert err_new <= max(5e-6, 2.0 * err_old), (err_new, err_old)


# ---- steps -----------------------------------------------------------------------------------------------------------------------
def _oracle_loss(task, params, cfg, x, y, lengths, sups):
    uniq, po = {}, {}
    for k, v in params.items():                                  # decoding_cells.l, l >= 2, alias decoding_cells.1: one leaf
        if id(v) not in uniq:
            uniq[id(v)] = v.clone().requires_grad_(True)
        po[k] = uniq[id(v)]
    if task == "ssl":
        lo = orc.regression_loss(y, orc.next_time_pred_forward(po, cfg, x, y, sups), loss_fn="MAE")
    else:
        logits = orc.classification_forward(po, cfg, x, lengths, sups)
        lo = orc.bce_with_logits(logits, y) if task == "detection" else orc.cross_entropy(logits, y)
    lo.backward()
    return lo, po


def _step_case(adj3d, task, graph, raw, b, t_in, t_out, device, seed=57, window=200):
    """TrainStep(use_fft=False, data_augment=True) on a model with input_dim = output_dim = 200 and oracle parameters, its inputs,
    and the oracle chain for a given set of draws"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    g = torch.Generator().manual_seed(seed)
    n = 19
    raw_x, raw_y = _signals(g, b, n, t_in * window), _signals(g, b, n, t_out * window)
    filt = "laplacian" if graph == "distance" else "dual_random_walk"
    classes = {"detection": 1, "classification": 4, "ssl": 1}[task]
    cfg = orc.DCRNNConfig(filter_type=filt, input_dim=window, output_dim=window, num_classes=classes)
    params = orc.init_params(cfg, "ssl" if task == "ssl" else "classification", seed=3)
    model = DCRNNModel_nextTimePred(make_args(cfg), device=device) if task == "ssl" else DCRNNModel_classification(make_args(cfg), classes, device=device)
    load(model, params, device)
    model.train()
    plain, refl = utils.compute_supports(adj3d, filt), utils.reflected_supports(adj3d, filt)
    kw = dict(raw_window=window, raw_mean=MEAN, raw_std=STD) if raw else dict(feature_mean=MEAN, feature_std=STD)
    torch.manual_seed(1234)                                       # the seed of the step's augmentation generator
    st = TrainStep(model, task=task, use_fft=False, data_augment=True, reflected_supports=refl if graph == "distance" else None, **kw)
    sup_in = [p_.unsqueeze(0).repeat(b, 1, 1).to(device) for p_ in plain] if graph == "distance" else None
    lengths = torch.full((b,), t_in, dtype=torch.int64)
    if task == "ssl":
        label = None
    elif task == "detection":
        label = (torch.rand(b, generator=g) > 0.5).float()
    else:
        label = torch.randint(0, classes, (b,), generator=g)
    ready = lambda r: torch.from_numpy(oracle_windows(r.numpy(), window, None, None, MEAN, STD).astype(np.float32))     # noqa: E731
    x_in = raw_x if raw else ready(raw_x)
    y_in = (raw_y if raw else ready(raw_y)) if task == "ssl" else label

    def oracle(flags, perm, scale, at=None):
        """the oracle chain for the draws of one step (at: other parameters than the initial ones) -> (loss, leaves with gradients)"""
        pn, sn = perm.numpy(), scale.numpy().astype(np.float64)
        if raw:
            to_win = lambda r: oracle_windows(r.numpy(), window, pn, sn, MEAN, STD)     # noqa: E731
        else:       # ready windows: multiplying the signals in front of the scaler = w * s + (s - 1) * mean / std behind it
            to_win = lambda r: (np.stack([r.numpy().astype(np.float64)[i][:, pn[i], :] for i in range(b)]) * sn[:, None, None, None]     # noqa: E731
                                + ((sn - 1.0) * MEAN / STD)[:, None, None, None])
        x = torch.from_numpy(to_win(raw_x if raw else x_in).astype(np.float32))
        y = torch.from_numpy(to_win(raw_y if raw else y_in).astype(np.float32)) if task == "ssl" else label
        if graph == "distance":
            sups = [torch.stack([(refl[k] if flags[i] else plain[k]) for i in range(b)]) for k in range(len(plain))]
        else:                                                     # the graph of the un-augmented INPUT: raw rows, or the ready windows
            clips = oracle_windows(raw_x.numpy(), window) if raw else x_in.numpy().astype(np.float64)
            per = [utils.compute_supports(utils.correlation_graph(clips[i], top_k=3), filt) for i in range(b)]
            sups = [torch.stack([per[i][k] for i in range(b)]) for k in range(2)]
        return _oracle_loss(task, params if at is None else at, cfg, x, y, lengths, sups)

    return st, model, x_in.to(device), y_in.to(device), lengths.to(device), sup_in, oracle


def check_timedomain_step(device, adj3d, task="detection", graph="distance", raw=True, b=6, t_in=3, t_out=2):
    """`TrainStep(use_fft=False, data_augment=True)`, two `forward_backward` calls; the draws are read back (`last_augmentation`,
    `last_scale`) and handed to the oracle chain (numpy windows -> reflect -> * scale -> z-score, on x and for ssl on y -> host
    graph builders -> oracle model and criterion): loss within 2e-5 absolute, every parameter gradient within
    `assert_close_scaled(tol=1e-4)` (the criteria of `ssl_chain_suite.check_augmented_ssl_step`); the draws of the two steps differ,
    both coin outcomes occurred, `eval()` draws nothing.

    FAILS ON THE PARENT COMMIT: `TrainStep(use_fft=False)` is a TypeError there."""
    st, model, x_in, y_in, lengths, sup_in, oracle = _step_case(adj3d, task, graph, raw, b, t_in, t_out, device)
    draws = []
    for step in range(2):                                          # two steps: the generator advanced, the draws differ
        loss = st.forward_backward(x_in, y_in, lengths, sup_in)
        flags, perm, ls = (t.cpu() for t in st.last_augmentation)
        scale = st.last_scale.cpu()
        assert torch.equal(scale, torch.exp(ls)) or float((scale - torch.exp(ls)).abs().max()) < 1e-6
        draws.append(flags.tolist() + scale.tolist())
        lo, po = oracle(flags, perm, scale)
        print(f"time-domain step {task}/{graph}/{'raw' if raw else 'windows'} step {step}: loss {loss.item():.7f} oracle {lo.item():.7f}")
        assert abs(float(loss.item()) - float(lo.item())) < 2e-5, (float(loss.item()), float(lo.item()))
        for k, q in model.named_parameters():
            assert_close_scaled(q.grad.cpu().numpy(), po[k].grad.numpy(), f"time-domain step {task}/{graph}/d_{k}", tol=1e-4)
    assert draws[0] != draws[1]
    assert 0 < sum(draws[0][:b]) + sum(draws[1][:b]) < 2 * b       # both outcomes of the coin were exercised
    assert all(0.8 <= s < 1.2 + 1e-6 for s in draws[0][b:] + draws[1][b:])
    model.eval()                                                 # no augmentation outside training
    st.last_augmentation = st.last_scale = None
    st.forward_backward(x_in, y_in, lengths, sup_in)
    assert st.last_augmentation is None and st.last_scale is None


def _params_of(model):
    """the model's parameters as oracle leaves' sources (host copies; aliased entries stay one tensor)"""
    uniq, out = {}, {}
    for k, v in model.state_dict().items():
        if v.data_ptr() not in uniq:
            uniq[v.data_ptr()] = v.detach().cpu().clone()
        out[k] = uniq[v.data_ptr()]
    return out


def check_captured_timedomain_step(device, adj3d, b=6, t_in=3, t_out=2):
    """`capture()` of the raw SSL time-domain step (correlation graph) and three `replay_step()`s: every replay draws afresh and its
    loss is the oracle's for the draws read back (2e-5 absolute), on the parameters that replay started from."""
    st, model, x_in, y_in, lengths, sup_in, oracle = _step_case(adj3d, "ssl", "correlation", True, b, t_in, t_out, device)
    st.capture(x_in, y_in, None, sup_in)
    seen = []
    for r in range(3):
        before = _params_of(model)
        loss = float(st.replay_step().item())
        flags, perm, _ = (t.cpu().clone() for t in st.last_augmentation)
        scale = st.last_scale.cpu().clone()
        seen.append(flags.tolist() + scale.tolist())
        lo, _ = oracle(flags, perm, scale, before)
        print(f"captured time-domain ssl step replay {r}: loss {loss:.7f} oracle {lo.item():.7f} flags {flags.tolist()}")
        assert abs(loss - float(lo.item())) < 2e-5, (r, loss, float(lo.item()))
    assert seen[0] != seen[1] and seen[1] != seen[2] and seen[0] != seen[2]
    assert st.samples_seen == 3 * b and st.step_count == 3


def check_refusals(device):
    """operands that do not fit are refused loudly, at the operator, at `TrainStep` and at the C ABI (`eeg_dcrnn_last_error` names
    the cause); nothing is launched on an empty grid"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, _lib, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    z = lambda *s: torch.zeros(*s, device=device)     # noqa: E731
    n = 19
    ident = torch.arange(n, dtype=torch.int32, device=device).repeat(2, 1)
    one = torch.ones(2, device=device)
    for what, call, msg in (
            ("raw input of a broken window", lambda: ops.window_features(z(2, n, 250), 200, 0.0, 1.0), "raw input signals must be"),
            ("raw input 2-D", lambda: ops.window_features(z(n, 400), 200, 0.0, 1.0), "raw input signals must be"),
            ("window not a multiple of 4", lambda: ops.window_features(z(2, n, 404), 202, 0.0, 1.0), "window=202 unsupported"),
            ("zero std", lambda: ops.window_features(z(2, n, 400), 200, 0.0, 0.0), "std must be non-zero"),
            ("perm of another shape", lambda: ops.window_features(z(2, n, 400), 200, 0.0, 1.0, perm=ident[:1]), "perm has shape"),
            ("scale of another batch", lambda: ops.window_features(z(2, n, 400), 200, 0.0, 1.0, scale=z(3)), "scale has 3"),
            ("raw target of another batch", lambda: ops.window_features_pair(z(2, n, 400), z(3, n, 200), 200, 0.0, 1.0), "raw target signals must be"),
            ("raw target of another node count", lambda: ops.window_features_pair(z(2, n, 400), z(2, 7, 200), 200, 0.0, 1.0), "raw target signals must be"),
            ("raw target of a broken window", lambda: ops.window_features_pair(z(2, n, 400), z(2, n, 250), 200, 0.0, 1.0), "raw target signals must be"),
            ("empty raw target", lambda: ops.window_features_pair(z(2, n, 400), z(2, n, 0), 200, 0.0, 1.0), "raw target signals must be"),
            ("pair: zero std", lambda: ops.window_features_pair(z(2, n, 400), z(2, n, 200), 200, 0.0, 0.0), "std must be non-zero"),
            ("pair: scale of another batch", lambda: ops.window_features_pair(z(2, n, 400), z(2, n, 200), 200, 0.0, 1.0, scale=z(5)), "scale has 5"),
            ("augment: perm of another shape", lambda: ops.augment_windows(z(2, 3, n, 8), None, ident[:1], one, 0.0, 1.0), "perm has shape"),
            ("augment: scale of another batch", lambda: ops.augment_windows(z(2, 3, n, 8), None, ident, z(5), 0.0, 1.0), "scale has 5"),
            ("augment: target of another width", lambda: ops.augment_windows(z(2, 3, n, 8), z(2, 2, n, 12), ident, one, 0.0, 1.0), "target windows must be"),
            ("augment: target of another batch", lambda: ops.augment_windows(z(2, 3, n, 8), z(3, 2, n, 8), ident, one, 0.0, 1.0), "target windows must be"),
            ("augment: D not a multiple of 4", lambda: ops.augment_windows(z(2, 3, n, 6), None, ident, one, 0.0, 1.0), "window=6 unsupported"),
            ("augment: zero std", lambda: ops.augment_windows(z(2, 3, n, 8), None, ident, one, 0.0, 0.0), "std must be non-zero"),
            ("augment: no draws", lambda: ops.augment_windows(z(2, 3, n, 8), None, None, one, 0.0, 1.0), "perm|Tensor"),
            ("rows: L not a multiple of 4", lambda: ops.correlation_supports_raw(z(2, n, 402)), "rows of 402 samples"),
            ("rows: 4-D", lambda: ops.correlation_supports_raw(z(2, 2, n, 200)), "raw signals must be"),
            ("rows: empty batch", lambda: ops.correlation_supports_raw(z(0, n, 400)), "empty"),
            ("rows: too many nodes", lambda: ops.correlation_supports_raw(z(2, 40, 400)), "num_nodes=40"),
            ("rows: top_k", lambda: ops.correlation_supports_raw(z(2, n, 400), top_k=n), "top_k=19"),
    ):
        with pytest.raises((RuntimeError, TypeError), match=msg):
            call()
            pytest.fail(f"{what}: accepted")
    # TrainStep: ready windows need the scaler's mean AND std; a raw SSL target must be whole windows
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=200, output_dim=200)
    model = DCRNNModel_classification(make_args(cfg), 1, device=device).to(device)
    for kw in (dict(), dict(feature_std=2.0), dict(feature_mean=1.0)):
        with pytest.raises(ValueError, match="feature_mean and feature_std"):
            TrainStep(model, task="detection", use_fft=False, data_augment=True, **kw)
    st = TrainStep(model, task="ssl", use_fft=False, raw_window=200)
    for bad_y in (z(2, n, 250), z(2, 2, n, 200)):
        with pytest.raises(ValueError, match=r"RAW target \(B, num_nodes, Ty\*200\)"):
            st.forward_backward(z(2, n, 400), bad_y, None, None)
    # C ABI: null operands, degenerate sizes
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    x, y, ox, oy, sc = z(2, n, 400), z(2, n, 200), z(2, 2, n, 200), z(2, 1, n, 200), one
    single = lambda *a: lib.query("eeg_dcrnn_window_features", *a)             # noqa: E731
    pair = lambda *a: lib.query("eeg_dcrnn_window_features_pair", *a)          # noqa: E731
    aug = lambda *a: lib.query("eeg_dcrnn_augment_windows", *a)                # noqa: E731
    rows = lambda *a: lib.query("eeg_dcrnn_corr_graph_rows", *a)               # noqa: E731
    refused(single(p(x), 2, n, 2, 200, None, None, 0.0, 1.0, None, None), "window_features: null output")
    refused(single(None, 2, n, 2, 200, None, None, 0.0, 1.0, p(ox), None), "window_features: null input")
    refused(single(p(x), 0, n, 2, 200, None, None, 0.0, 1.0, p(ox), None), "window_features: empty input")
    refused(single(p(x), 2, n, 0, 200, None, None, 0.0, 1.0, p(ox), None), "window_features: empty input")
    refused(single(p(x), 2, n, 2, 202, None, None, 0.0, 1.0, p(ox), None), "window=202 unsupported")
    refused(single(p(x), 2, n, 2, 200, None, None, 0.0, 0.0, p(ox), None), "std must be non-zero")
    refused(single(p(x), 2, n, 2, 200, None, None, 0.0, 1.0, p(x), None), "in-place")
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 1.0, p(ox), None, None), "window_features_pair: null output")
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 1.0, None, p(oy), None), "window_features_pair: null output")
    refused(pair(p(x), None, 2, n, 2, 1, 200, None, None, 0.0, 1.0, p(ox), p(oy), None), "window_features_pair: null input")
    refused(pair(p(x), p(y), 2, n, 2, 0, 200, None, None, 0.0, 1.0, p(ox), p(oy), None), "window_features_pair: empty input")
    refused(pair(p(x), p(y), 2, n, 2, 1, 6, None, None, 0.0, 1.0, p(ox), p(oy), None), "window=6 unsupported")
    refused(pair(p(x), p(y), 2, n, 2, 1, 200, None, None, 0.0, 0.0, p(ox), p(oy), None), "std must be non-zero")
    fx, fy, gx, gy = z(2, 2, n, 8), z(2, 1, n, 8), z(2, 2, n, 8), z(2, 1, n, 8)
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sc), p(sc), None, p(gy), None), "augment_windows: null output")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sc), p(sc), p(gx), None, None), "augment_windows: null output")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, None, p(sc), p(sc), p(gx), p(gy), None), "augment_windows: null input / perm / factors")
    refused(aug(p(fx), p(fy), 2, 2, 0, n, 8, p(ident), p(sc), p(sc), p(gx), p(gy), None), "disagree")
    refused(aug(p(fx), None, 2, 2, 1, n, 8, p(ident), p(sc), p(sc), p(gx), p(gy), None), "disagree")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 8, p(ident), p(sc), p(sc), p(fx), p(gy), None), "in-place")
    refused(aug(p(fx), p(fy), 2, 2, 1, n, 6, p(ident), p(sc), p(sc), p(gx), p(gy), None), "window=6 unsupported")
    refused(aug(p(fx), p(fy), 0, 2, 1, n, 8, p(ident), p(sc), p(sc), p(gx), p(gy), None), "augment_windows: empty input")
    a1, a2, a3, ws = z(2, n, n), z(2, n, n), z(2, n, n), z(2 * 768 * 4)
    assert lib.query("eeg_dcrnn_corr_graph_rows_ws_floats", 0, 1, 400) == 0 and lib.query("eeg_dcrnn_corr_graph_rows_ws_floats", 2, 1, 0) == 0
    assert lib.query("eeg_dcrnn_corr_graph_rows_ws_floats", 2, 1, 400) <= ws.numel()
    refused(rows(p(x), 2, n, 1, 400, 0, 3, p(a1), None, p(a3), p(ws), None), "corr_graph_rows: null output")
    refused(rows(None, 2, n, 1, 400, 0, 3, p(a1), p(a2), p(a3), p(ws), None), "corr_graph_rows: null input")
    refused(rows(p(x), 2, n, 1, 400, 0, 3, p(a1), p(a2), p(a3), None, None), "corr_graph_rows: null input")
    refused(rows(p(x), 0, n, 1, 400, 0, 3, p(a1), p(a2), p(a3), p(ws), None), "corr_graph_rows: empty")
    refused(rows(p(x), 2, n, 0, 400, 0, 3, p(a1), p(a2), p(a3), p(ws), None), "corr_graph_rows: empty")
    refused(rows(p(x), 2, n, 1, 402, 0, 3, p(a1), p(a2), p(a3), p(ws), None), "402 floats unsupported")
    refused(rows(p(x), 2, 33, 1, 400, 0, 3, p(a1), p(a2), p(a3), p(ws), None), "num_nodes=33")
    refused(rows(p(x), 2, n, 2, 200, 100, 3, p(a1), p(a2), p(a3), p(ws), None), "piece stride 100")
    refused(rows(p(x), 2, n, 1, 400, 0, n, p(a1), p(a2), p(a3), p(ws), None), "top_k=19")
