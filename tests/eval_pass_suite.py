"""Checks of the evaluation pass on the device (eeg_gnn_ssl_amd/evaluation.py, csrc/kernels_eval.h): the per-clip scores kernel
(`ops.eval_scores`), the scores of a pool (`ops.eval_metrics`) against sklearn, `DeviceEvaluator` against a hand-made eager run and
against the existing `evaluate`, the inputs the existing helpers cannot evaluate (raw pools, time-domain pools, the graph of the
unpadded clip), the absence of side effects, the captured pass, and refusals.  As in device_epoch_suite.py the same functions run on
the GPU library and on the emulator build of the same kernel sources (tests/test_eval_pass.py).

Each check FAILS ON THE PARENT COMMIT: `ops.eval_scores`, `ops.eval_metrics`, `TrainStep.evaluator` and `DeviceEvaluator` do not exist
there."""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import assert_close, load, make_args

P, B, T, D, W, N = 23, 4, 3, 8, 8, 19
PROB_RTOL = 5e-7                  # one expf, one add and one divide: about 8 ulp of float32 (2^-24 each, and expf's own few)
PROB_ATOL = 2.0 ** -126           # below the smallest normal float32 the spacing is absolute, and expf(100) overflows: sigmoid(-100) = 0


# ---- 1. the scores kernel -------------------------------------------------------------------------------------------------------------
def _guarded(shape, device, fill=-5.0, sentinel=-77.0):
    """a float32 buffer between one sentinel row in front and one behind -> (view, intact())"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), sentinel, dtype=torch.float32, device=device)
    buf[1:-1] = fill

    def intact():
        return bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    return buf[1:-1], intact


def check_scores_kernel(device):
    """`ops.eval_scores` for C = 1 and C = 4: B = 5 slots with clip_w = [1, 1, 1, 0, 0] over a pool of P = 7, logits with +-100; the
    cursor (as the gather leaves it: c0 + B*world) puts the batch at the start, across the end (slot 2 would be position 7: refused by
    the kernel's own bound, its weight is 1), wholly behind the end, at negative positions, partly negative, and far away; ranks (0, 1)
    and (1, 2).  Written slots: probabilities against the float64 sigmoid / softmax of the same logits (rtol 5e-7), losses bit for bit
    `ops.bce_with_logits` / `ops.cross_entropy` of that clip as a batch of one.  Every other entry keeps its fill value and the
    sentinel rows around the buffers stay intact."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(5)
    pool, b = 7, 5
    clip_w = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0]).to(device)
    cases = 0
    for c in (1, 4):
        logits = torch.randn(b, c, generator=g) * 3
        logits[0, 0], logits[1, c - 1], logits[2, 0] = 100.0, -100.0, -100.0 if c == 1 else 100.0
        if c == 1:
            labels = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0])
            want_p = torch.sigmoid(logits.double()).view(-1)
        else:
            labels = torch.tensor([0, 3, 1, 2, 2, 0, 3])
            want_p = torch.softmax(logits.double(), dim=1)
        lg, lab = logits.to(device), labels.to(device)
        for rank, world in ((0, 1), (1, 2)):
            for c0 in (0, 5, 7, -8, -1, 2 ** 62 + 5, -2 ** 63 + 3):
                cursor = torch.tensor([c0], dtype=torch.int64) + b * world          # (wraps like the device's int64 would)
                probs, p_ok = _guarded((pool,) if c == 1 else (pool, c), device)
                losses, l_ok = _guarded((pool,), device)
                ops.eval_scores(lg, lab, clip_w, cursor.to(device), probs, losses, rank, world)
                assert p_ok() and l_ok(), (c, rank, world, c0)
                written = {}
                for slot in range(b):
                    pos = c0 + rank * b + slot
                    if clip_w[slot] != 0 and 0 <= pos < pool:
                        written[pos] = slot
                got_p, got_l = probs.cpu(), losses.cpu()
                for pos in range(pool):
                    tag = (c, rank, world, c0, pos)
                    if pos not in written:
                        assert bool((got_p[pos] == -5.0).all()) and float(got_l[pos]) == -5.0, tag
                        continue
                    s = written[pos]
                    err = (got_p[pos].double() - want_p[s]).abs()
                    assert bool((err <= PROB_RTOL * want_p[s] + PROB_ATOL).all()), (tag, got_p[pos], want_p[s])
                    if c == 1:
                        one = ops.bce_with_logits(lg[s:s + 1].view(-1), lab[pos:pos + 1])
                    else:
                        one = ops.cross_entropy(lg[s:s + 1], lab[pos:pos + 1])
                    assert got_l[pos].view(torch.int32).item() == one.cpu().view(torch.int32).item(), (tag, got_l[pos], one)
                    cases += 1
    assert cases >= 2 * (3 + 2 + 2 + 3)          # start: 3, across: 2, partly negative: 2 per class on one rank, + the second rank's


# ---- 2. the metrics kernel against sklearn --------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2, 3, 2047, 2048, 2049, 4095, 4096, 4097, 100003)     # 2048 = the LDS tile, 4096 = the first size with a global step


@functools.lru_cache(maxsize=None)
def _detection_cases():
    """(name, prob float32, label float32, auroc, searched threshold, score dict at it) -- the references, computed once:
    `metrics.roc_auc_score`, `utils.thresh_max_f1`, `utils.eval_dict` on the float32 scores"""
    from sklearn import metrics
    from eeg_gnn_ssl_amd import utils
    rng = np.random.default_rng(0)
    draws = []
    for d in range(400):
        p = int(rng.integers(5, 400))
        rate = (0.1, 0.5)[int(rng.integers(0, 2))]
        y = (rng.random(p) < rate).astype(np.float32)
        logit = rng.standard_normal(p) * (1, 5, 30)[int(rng.integers(0, 3))] + y
        if d % 3 == 0:
            logit = np.round(logit)
        if len(set(y.tolist())) == 2:
            draws.append((f"draw {d}", logit, y))
    for p in SORT_SIZES:
        y = (rng.random(p) < 0.5).astype(np.float32)
        y[0] = 1.0
        if p > 1:
            y[1] = 0.0
        draws.append((f"P={p}", np.round(rng.standard_normal(p) * 5 + y, 1 if p < 5000 else 3), y))
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, logit, y in draws:
            prob = torch.sigmoid(torch.tensor(logit, dtype=torch.float32)).numpy()
            yi = y.astype(int)
            thresh = utils.thresh_max_f1(y_true=yi, y_prob=prob)
            scores, _, _ = utils.eval_dict(y_pred=(prob > float(thresh)).astype(int), y=yi, y_prob=prob, average="binary")
            out.append((name, prob, y, np.float32(thresh), scores))
    return out


def _same(a, b, tol=1e-12):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def check_metrics_detection(device):
    """`ops.eval_metrics` + `scores_from_record` on 400 draws of default_rng(0) (P in 5..399, positive rate 0.1 / 0.5, logit = N(0,1) *
    {1, 5, 30} + y, every third rounded: heavy ties and saturated 0 / 1; one-class draws skipped) and P in {1, 2, 3} and around the
    sort's sizes, P = 100003: AUROC within 1e-12 of `roc_auc_score`, the searched threshold EQUAL as float32 to `utils.thresh_max_f1`,
    acc / F1 / precision / recall within 1e-12 of `utils.eval_dict` at that threshold -- in every case; a given threshold 0.5 (strict
    `prob > thresh`, probabilities of exactly 0.5 among the rounded draws); P = 1 is one class: AUROC as eval_dict has it there.
    (Draws 24 and 327 hold two candidates whose F1 tie as rationals, 0.2, and differ in the last bit as the reference computes them:
    a kernel that compares exactly picks the lower threshold there, `thresh_max_f1` the higher.)"""
    from eeg_gnn_ssl_amd import ops, utils
    from eeg_gnn_ssl_amd.evaluation import scores_from_record
    cases = _detection_cases()
    assert len(cases) >= 390 + len(SORT_SIZES)
    worst = 0.0
    for name, prob, y, thresh, want in cases:
        pt, yt = torch.from_numpy(prob).to(device), torch.from_numpy(y).to(device)
        losses = torch.zeros(len(y), device=device)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = scores_from_record(ops.eval_metrics(pt, yt, losses, search=True), "detection")
        assert np.float32(got["best_thresh"]) == thresh, (name, got["best_thresh"], thresh)
        for k in ("acc", "F1", "precision", "recall", "auroc"):
            assert _same(got[k], want[k]), (name, k, got[k], want[k])
        if not np.isnan(want["auroc"]):
            worst = max(worst, abs(got["auroc"] - want["auroc"]))
    print(f"eval_metrics detection: {len(cases)} cases, max |auroc - sklearn| = {worst:.3e}")
    for name, prob, y, _, _ in cases[:40]:
        pt, yt = torch.from_numpy(prob).to(device), torch.from_numpy(y).to(device)
        got = scores_from_record(ops.eval_metrics(pt, yt, torch.zeros(len(y), device=device), search=False, thresh=0.5), "detection", 0.5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want, _, _ = utils.eval_dict(y_pred=(prob.astype(np.float64) > 0.5).astype(int), y=y.astype(int), y_prob=prob, average="binary")
        assert got["best_thresh"] == 0.5 and all(_same(got[k], want[k]) for k in ("acc", "F1", "precision", "recall", "auroc")), (name, got, want)


def check_metrics_classification(device):
    """C = 4 confusion matrices against `sklearn.metrics.confusion_matrix` and the weighted scores of `utils.eval_dict`: random rows,
    rows with tied maxima (first arg-max), a class never predicted, a class absent from the labels; the loss is sum(losses) / P"""
    from sklearn import metrics
    from eeg_gnn_ssl_amd import ops, utils
    from eeg_gnn_ssl_amd.evaluation import scores_from_record
    g = torch.Generator().manual_seed(9)
    for p, never, absent in ((57, None, None), (300, 2, None), (41, None, 3), (1500, 1, 0)):
        logits = torch.randn(p, 4, generator=g) * 2
        if never is not None:
            logits[:, never] = -50.0
        prob = torch.softmax(logits, dim=1)
        prob[::7] = torch.tensor([0.25, 0.25, 0.25, 0.25]) if never is None else prob[::7]      # tied rows: the first arg-max wins
        y = torch.randint(0, 4, (p,), generator=g)
        if absent is not None:
            y[y == absent] = (absent + 1) % 4
        losses = torch.rand(p, generator=g)
        rec = ops.eval_metrics(prob.to(device), y.to(device), losses.to(device)).cpu()
        pred = np.argmax(prob.numpy(), axis=1)
        cm = metrics.confusion_matrix(y.numpy(), pred, labels=[0, 1, 2, 3])
        assert np.array_equal(rec[ops.EVAL_RECORD_HEAD:].numpy().reshape(4, 4), cm), (p, never, absent)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want, _, _ = utils.eval_dict(y_pred=pred, y=y.numpy(), average="weighted")
        got = scores_from_record(rec, "classification", 0.5)
        assert list(got) == ["loss", "acc", "F1", "recall", "precision", "best_thresh"]
        assert all(_same(got[k], want[k]) for k in ("acc", "F1", "precision", "recall")), (got, want)
        assert abs(got["loss"] - float(losses.double().sum()) / p) <= 1e-12
        if never is not None:
            assert cm[:, never].sum() == 0
        if absent is not None:
            assert cm[absent].sum() == 0


def check_metrics_flags_and_reproducibility(device):
    """a NaN score, a score above 1, a label 2 (detection) and a class 4 of 4 (classification) each raise ValueError; two runs on the
    same inputs give a bit-identical record, and so does a run in other buffers"""
    from eeg_gnn_ssl_amd import ops
    from eeg_gnn_ssl_amd.evaluation import scores_from_record
    g = torch.Generator().manual_seed(13)
    p = 3000
    prob, y = torch.rand(p, generator=g), (torch.rand(p, generator=g) < 0.3).float()
    losses = torch.rand(p, generator=g)
    d = lambda t: t.to(device)     # noqa: E731
    ws, rec = ops.eval_metrics_buffers(p, 1, device)
    first = ops.eval_metrics(d(prob), d(y), d(losses), True, 0.5, ws, rec).cpu().clone()
    again = ops.eval_metrics(d(prob), d(y), d(losses), True, 0.5, ws, rec).cpu().clone()
    fresh = ops.eval_metrics(d(prob), d(y), d(losses), True).cpu()
    assert torch.equal(first, again) and torch.equal(first, fresh)
    assert int(first[0]) == p and int(first[1]) + int(first[2]) == p and int(first[5] + first[6] + first[7] + first[8]) == p
    assert abs(scores_from_record(first, "detection")["loss"] - float(losses.double().sum()) / p) <= 1e-12
    for bad_prob, bad_label in ((float("nan"), None), (1.5, None), (-0.25, None), (None, 2.0)):
        pp, yy = prob.clone(), y.clone()
        if bad_prob is not None:
            pp[17] = bad_prob
        else:
            yy[17] = bad_label
        with pytest.raises(ValueError, match=r"1 labels outside" if bad_prob is None else r"and 1 probabilities outside"):
            scores_from_record(ops.eval_metrics(d(pp), d(yy), d(losses), True), "detection")
    soft = torch.softmax(torch.randn(50, 4, generator=g), dim=1)
    cls = torch.randint(0, 4, (50,), generator=g)
    cls[3] = 4
    with pytest.raises(ValueError, match=r"1 labels outside"):
        scores_from_record(ops.eval_metrics(d(soft), d(cls), d(torch.zeros(50))), "classification")
    cls[3] = 0
    soft[5, 1] = float("nan")
    with pytest.raises(ValueError, match=r"1 probabilities outside"):
        scores_from_record(ops.eval_metrics(d(soft), d(cls), d(torch.zeros(50))), "classification")
    # no positive clip: the search has no candidate, as utils.thresh_max_f1 has none
    with pytest.raises(ValueError, match="no candidate"):
        scores_from_record(ops.eval_metrics(d(prob), d(torch.zeros(p)), d(losses), True), "detection")


# ---- 3. / 4. the pass -----------------------------------------------------------------------------------------------------------------
def _case(kind, adj3d, device, units):
    """-> (model, TrainStep keywords, task, dataset, supports, by_hand(i, j) -> (x, supports) of clips i..j for `evaluate`)"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DeviceDataset, ops, utils
    g = torch.Generator().manual_seed(41)
    lens = None
    if kind == "detection":                 # features, the shared Laplacian graph: the spectral path at 64 units
        cfg = orc.DCRNNConfig(filter_type="laplacian", input_dim=D, num_classes=1, rnn_units=units)
        x = torch.randn(P, T, N, D, generator=g).to(device)
        supports, kw, task = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")], dict(), "detection"
        hand = lambda i, j: (x[i:j], supports)     # noqa: E731
    elif kind == "classification":          # C = 4, the dual random-walk supports of the distance graph: the general path
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=D, num_classes=4, rnn_units=units)
        x = torch.randn(P, T, N, D, generator=g).to(device)
        shared = [s.to(device) for s in utils.compute_supports(adj3d, "dual_random_walk")]
        supports, kw, task = shared, dict(), "classification"
        hand = lambda i, j: (x[i:j], shared)     # noqa: E731
    elif kind == "raw_fft":                 # raw signals -> log|FFT| -> z-score, correlation graph of the un-standardised features
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W // 2, num_classes=1, rnn_units=units)
        x = torch.randn(P, N, T * W, generator=g).to(device)
        supports, kw, task = None, dict(raw_window=W, raw_mean=0.3, raw_std=1.7), "detection"

        def hand(i, j):
            feat_raw, xf = ops.fft_features(x[i:j], window=W, mean=0.3, std=1.7)
            return xf, ops.correlation_supports(feat_raw, top_k=3)
    elif kind == "time_domain":             # raw signals -> windows -> z-score, correlation graph of the raw rows
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W, num_classes=1, rnn_units=units)
        x = torch.randn(P, N, T * W, generator=g).to(device)
        supports, kw, task = None, dict(raw_window=W, raw_mean=0.3, raw_std=1.7, use_fft=False), "detection"
        hand = lambda i, j: (ops.window_features(x[i:j], W, 0.3, 1.7), ops.correlation_supports_raw(x[i:j], top_k=3, window=W))     # noqa: E731
    else:                                   # "varlen": feature clips with a length pool, the graph of the UNPADDED clip
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=D, num_classes=4, rnn_units=units)
        x = torch.randn(P, T, N, D, generator=g).to(device)         # (whatever lies behind a clip's length stays: the graph must not see it)
        lens = torch.randint(1, T + 1, (P,), generator=g).to(device)
        supports, kw, task = None, dict(padding_val=0.0), "classification"
        hand = lambda i, j: (x[i:j], ops.correlation_supports(x[i:j], top_k=3, lengths=lens[i:j]))     # noqa: E731
    if task == "detection":
        y = (torch.rand(P, generator=g) < 0.5).float().to(device)
    else:
        y = torch.randint(0, 4, (P,), generator=g).to(device)
    model = DCRNNModel_classification(make_args(cfg), cfg.num_classes, device=device)
    load(model, orc.init_params(cfg, "classification", seed=6), device)
    return model, kw, task, DeviceDataset(x, y, lens), supports, hand


def _full_lens(ds, count, device):
    return torch.full((count,), T, dtype=torch.int64, device=device)


def _by_hand_batches(ds, hand, device):
    """the sequential batches `evaluate` takes (the last one holds 3 clips), data side made by hand"""
    out = []
    for i in range(0, P, B):
        j = min(i + B, P)
        x, sup = hand(i, j)
        out.append((x, ds.y[i:j], ds.seq_lengths[i:j] if ds.seq_lengths is not None else _full_lens(ds, j - i, device), sup))
    return out


def _against_evaluate(ev, res, model, batches, task, what, probs=True, **kw):
    """`DeviceEvaluator` against the existing helpers on the same clips: probabilities and loss at parity_suite's tolerance (the last
    batch has 3 clips there and 4 here: another kernel instance may serve it), the same keys in the same order, and the scores --
    counts over 23 clips -- equal"""
    from eeg_gnn_ssl_amd.train_step import evaluate, predict
    want = evaluate(model, batches, task=task, **kw)
    if probs:
        assert_close(ev.probs.cpu().numpy(), predict(model, batches, task=task)[0], f"{what}: probabilities")
    assert list(res) == list(want), (what, list(res), list(want))
    assert_close(np.array([res["loss"]]), np.array([want["loss"]]), f"{what}: loss")
    for k in want:
        if k not in ("loss", "best_thresh"):
            assert _same(res[k], want[k]), (what, k, dict(res), dict(want))
    assert abs(res["best_thresh"] - want["best_thresh"]) <= 1e-5, (what, res["best_thresh"], want["best_thresh"])
    print(f"{what}: {dict(res)}")


def check_pass(device, adj3d, kind, units):
    """kind "detection" (shared Laplacian graph, 64 units: the spectral path) / "classification" (C = 4, the general path):
    `ev.probs` / `ev.losses` of an eager pass equal, bit for bit, a hand-made eager run of the same six wrapped batches (batch k =
    clips (k*B + b) mod P) through `model` and the loss operators; the pass agrees with `evaluate(model, ds.batches(B, supports))`;
    the score dictionary has its keys and order; the threshold search (is_test=True, eval_set="dev") runs here, a given best_thresh
    in `check_new_ground`."""
    from eeg_gnn_ssl_amd import ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    model, kw, task, ds, supports, hand = _case(kind, adj3d, device, units)
    st = TrainStep(model, task=task, **kw)
    before = ops.spectral_layer_calls
    ev = st.evaluator(ds, B, supports=supports)
    res = ev.run(is_test=True, eval_set="dev", capture=False)
    if kind == "detection" and units == 64:
        assert ops.spectral_layer_calls > before, "the shared 2-D graph takes the spectral form"
    if kind == "classification":
        assert ops.spectral_layer_calls == before, "the dual random-walk supports take the general path"
    assert ev.sampler.steps_per_epoch == 6 and int(ev.sampler.cursor.item()) == 6 * B and st.sampler is None
    # the hand-made run
    c = ev.classes
    probs = torch.full_like(ev.probs, -1.0)
    losses = torch.full_like(ev.losses, -1.0)
    model.eval()
    with torch.no_grad():
        for k in range(6):
            idx = (torch.arange(B, device=device) + k * B) % P
            logits = model(ds.x[idx], _full_lens(ds, B, device), supports).view(B, c)
            valid = (torch.arange(B) + k * B) < P
            ops.eval_scores(logits, ds.y, valid.float().to(device), torch.tensor([(k + 1) * B], device=device), probs, losses)
            for b in range(B):
                if valid[b]:
                    pos = k * B + b
                    one = (ops.bce_with_logits(logits[b], ds.y[pos:pos + 1]) if c == 1 else ops.cross_entropy(logits[b:b + 1], ds.y[pos:pos + 1]))
                    assert torch.equal(one.reshape(()), ev.losses[pos]), (kind, pos)
    model.train()
    assert torch.equal(probs, ev.probs) and torch.equal(losses, ev.losses), kind
    assert bool(((ev.probs >= 0) & (ev.probs <= 1)).all())
    batches = list(ds.batches(B, supports))
    _against_evaluate(ev, res, model, batches, task, f"pass {kind} (search)", is_test=True, eval_set="dev")
    if kind == "classification":            # (the given threshold on a detection pool: check_new_ground, 16 units)
        res2 = ev.run(best_thresh=0.4, capture=False)
        assert torch.equal(probs, ev.probs) and torch.equal(losses, ev.losses)
        _against_evaluate(ev, res2, model, batches, task, f"pass {kind} (best_thresh=0.4)", probs=False, best_thresh=0.4)
        assert res2["best_thresh"] == 0.4
    assert model.training


def check_new_ground(device, adj3d, kind, units=16):
    """what `evaluate` cannot be handed directly: kind "raw_fft" (raw pool, raw_window = 8, supports=None), "time_domain"
    (use_fft=False), "varlen" (classification, length pool, padding_val = 0.0, supports=None).  The pass equals `evaluate` fed features
    / windows and graphs made by hand, batch by batch (`ops.fft_features` + `ops.correlation_supports(feat_raw)`;
    `ops.window_features` + `ops.correlation_supports_raw`; `ops.correlation_supports(x, lengths=lens)`).  For "varlen" the graph
    WITHOUT lengths -- what `evaluate(supports=None)` builds -- gives other probabilities: the lengths matter in this case."""
    from eeg_gnn_ssl_amd.train_step import TrainStep, predict
    model, kw, task, ds, supports, hand = _case(kind, adj3d, device, units)
    st = TrainStep(model, task=task, **kw)
    ev = st.evaluator(ds, B, supports=None)
    res = ev.run(is_test=True, eval_set="dev", capture=False)
    batches = _by_hand_batches(ds, hand, device)
    _against_evaluate(ev, res, model, batches, task, f"pass {kind}", is_test=True, eval_set="dev")
    if kind == "raw_fft":                   # a given threshold instead of the search
        first = ev.probs.clone()
        res2 = ev.run(best_thresh=0.4, capture=False)
        assert torch.equal(first, ev.probs) and res2["best_thresh"] == 0.4
        _against_evaluate(ev, res2, model, batches, task, f"pass {kind} (best_thresh=0.4)", probs=False, best_thresh=0.4)
    if kind == "varlen":
        padded, _ = predict(model, list(ds.batches(B, None)), task=task)
        assert np.abs(padded - ev.probs.cpu().numpy()).max() > 1e-3, "the graph of the padded clip differs: the case tells them apart"


# ---- 5. no side effects ----------------------------------------------------------------------------------------------------------------
def check_no_side_effects(device, adj3d, units=16):
    """a `TrainStep(data_augment=True)` over a dropout model in train mode, one training step taken (a training sampler attached, Adam
    moments non-zero): after `run`, model.training, step_count / samples_seen and their device mirrors, the parameters, exp_avg*, the
    augmentation and dropout generator states and the training sampler (object and cursor) are what they were, and the scores equal
    those of a step without augmentation and without dropout over the same parameters"""
    import copy
    from eeg_gnn_ssl_amd import DCRNNModel_classification, EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    model, kw, task, ds, supports, _ = _case("detection", adj3d, device, units)
    args = copy.copy(make_args(orc.DCRNNConfig(filter_type="laplacian", input_dim=D, num_classes=1, rnn_units=units)))
    args.dropout = 0.5
    noisy = DCRNNModel_classification(args, 1, device=device)
    noisy.load_state_dict(model.state_dict())
    noisy.to(device).train()
    torch.manual_seed(3)
    st = TrainStep(noisy, task="detection", data_augment=True, feature_std=1.7)
    train_sampler = EpochSampler(P, B, 77, 0, 1, device=device)
    st.begin_epoch(0, 2, sampler=train_sampler)
    st.step_from(ds, train_sampler, supports)
    ev = st.evaluator(ds, B, supports=supports)

    def state():
        return (noisy.training, st.step_count, st.samples_seen, st.step_dev.clone(), st.samples_seen_dev.clone(), st.fp.flat.detach().clone(),
                st.exp_avg.clone(), st.exp_avg_sq.clone(), st._augment_rng.clone(), noisy._dropout_rng.clone(), train_sampler.cursor.clone(),
                train_sampler._host_cursor, id(st.sampler), st.lr)

    before = state()
    assert bool(st.exp_avg.abs().sum() > 0) and int(train_sampler.cursor.item()) == B and noisy.training
    res = ev.run(is_test=True, eval_set="dev", capture=False)
    for u, v in zip(before, state()):
        assert torch.equal(u, v) if torch.is_tensor(u) else u == v
    assert st.sampler is train_sampler
    # a twin without augmentation or dropout, same parameters
    plain = DCRNNModel_classification(make_args(orc.DCRNNConfig(filter_type="laplacian", input_dim=D, num_classes=1, rnn_units=units)), 1,
                                      device=device)
    plain.load_state_dict(noisy.state_dict())
    plain.to(device)
    ev2 = TrainStep(plain, task="detection").evaluator(ds, B, supports=supports)
    res2 = ev2.run(is_test=True, eval_set="dev", capture=False)
    assert torch.equal(ev.probs, ev2.probs) and torch.equal(ev.losses, ev2.losses) and torch.equal(ev.record, ev2.record)
    assert list(res.items()) == list(res2.items())


# ---- 6. the captured pass (GPU only) ---------------------------------------------------------------------------------------------------
def check_captured(device, adj3d):
    """the captured pass equals the eager pass bit for bit (probs, losses, record); after one training step between two passes the
    REPLAYED graph equals a fresh eager pass (the parameters are read in place); a second run replays the same graph"""
    from eeg_gnn_ssl_amd import EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    for kind in ("detection", "varlen"):
        model, kw, task, ds, supports, _ = _case(kind, adj3d, device, 64)
        st = TrainStep(model, task=task, **kw)
        model.train()
        eager, graph = st.evaluator(ds, B, supports=supports), st.evaluator(ds, B, supports=supports)
        r_e = eager.run(is_test=True, eval_set="dev", capture=False)
        r_g = graph.run(is_test=True, eval_set="dev", capture=True)
        assert torch.equal(eager.probs, graph.probs) and torch.equal(eager.losses, graph.losses) and torch.equal(eager.record, graph.record), kind
        assert list(r_e.items()) == list(r_g.items()) and model.training
        first, handle = graph.probs.clone(), graph._graph
        sampler = EpochSampler(P, B, 5, 0, 1, device=device)
        st.begin_epoch(0, 2, sampler=sampler)
        st.step_from(ds, sampler, supports)                          # the parameters move
        r_g2 = graph.run(is_test=True, eval_set="dev", capture=True)
        assert graph._graph is handle and not torch.equal(first, graph.probs), kind
        fresh = st.evaluator(ds, B, supports=supports)
        r_e2 = fresh.run(is_test=True, eval_set="dev", capture=False)
        assert torch.equal(fresh.probs, graph.probs) and torch.equal(fresh.losses, graph.losses) and torch.equal(fresh.record, graph.record), kind
        assert list(r_e2.items()) == list(r_g2.items())


def check_captured_beside_training_graph(device, adj3d):
    """a `capture_epoch` graph and the evaluation graph alive together: the training losses of two epochs with a captured pass between
    them equal, bit for bit, those of the same two epochs without"""
    from eeg_gnn_ssl_amd import EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    runs = []
    for with_pass in (False, True):
        model, kw, task, ds, supports, _ = _case("detection", adj3d, device, 64)
        model.train()
        torch.manual_seed(99)
        st = TrainStep(model, task=task, **kw)
        sampler = EpochSampler(P, B, 5, 0, 1, device=device)
        sampler.begin_epoch(0)
        keep = st.snapshot()
        st.capture_epoch(ds, sampler, supports, include_update=True)
        st.restore(keep)
        ev = st.evaluator(ds, B, supports=supports)
        losses = []
        for e in range(2):
            st.begin_epoch(e, 2)
            losses += [st.replay_step().clone() for _ in range(sampler.steps_per_epoch)]
            if with_pass and e == 0:
                res = ev.run(is_test=True, eval_set="dev", capture=True)
                assert np.isfinite(res["loss"]) and int(sampler.cursor.item()) == sampler.steps_per_epoch * B
        runs.append((torch.stack(losses), st.fp.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].unique().numel() == runs[0][0].numel()


# ---- 7. two ranks: the pools of the worker and of the single process ---------------------------------------------------------------------
def two_rank_case(adj3d, clips, device="cpu"):
    """(TrainStep, dataset of the first `clips` clips, supports) of the two-rank check: built alike in every process"""
    from eeg_gnn_ssl_amd import DeviceDataset
    from eeg_gnn_ssl_amd.train_step import TrainStep
    model, kw, task, ds, supports, _ = _case("detection", adj3d, device, 16)
    return TrainStep(model, task=task, **kw), DeviceDataset(ds.x[:clips].contiguous(), ds.y[:clips].contiguous()), supports


# ---- 8. refusals, operator registration ------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d):
    """task="ssl" (the message names evaluate_ssl), batch_size*world > P, pools on another device, P over the limit, a label pool of
    the wrong dtype, padding_val without a length pool, capture without HIP graphs; the operators refuse wrong dtype, shape and device
    before the call; the C entry points refuse null pointers, P over the limit and a label size that does not fit C"""
    import ctypes
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, DeviceDataset, _lib, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    model, kw, task, ds, supports, _ = _case("detection", adj3d, device, 16)
    st = TrainStep(model, task=task)
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=D, output_dim=D, rnn_units=16)
    ssl = DCRNNModel_nextTimePred(make_args(cfg), device=device)
    ssl.to(device)
    with pytest.raises(ValueError, match=r"task='ssl'.*evaluate_ssl"):
        TrainStep(ssl, task="ssl").evaluator(ds, B)
    with pytest.raises(ValueError, match=r"batch_size\*world = 12\*2 clips per step, the pool holds P=23"):
        st.evaluator(ds, 12, rank=0, world=2)
    with pytest.raises(ValueError, match=r"DeviceEvaluator: dataset on meta"):
        st.evaluator(DeviceDataset(torch.zeros(P, T, N, D, device="meta"), torch.zeros(P, device="meta")), B)
    big = ops.EVAL_MAX_CLIPS + 1
    with pytest.raises(ValueError, match=rf"P={big} clips, one pass takes at most {ops.EVAL_MAX_CLIPS}"):
        st.evaluator(DeviceDataset(z(big, 1, 1, 4), z(big)), B)
    with pytest.raises(ValueError, match=r"labels \(P,\) as torch.float32, got torch.int64"):
        st.evaluator(DeviceDataset(ds.x, z(P, dtype=torch.int64)), B)
    with pytest.raises(ValueError, match=r"padding_val.*seq_lengths"):
        TrainStep(model, task=task, padding_val=0.0).evaluator(ds, B)
    if device == "cpu":
        with pytest.raises(RuntimeError, match=r"capture=True\) needs HIP graphs"):
            st.evaluator(ds, B, supports=supports).run()
    # the operators
    lg, lab, cw, cur, pr, ls = z(B, 1), z(P), z(B), z(1, dtype=torch.int64), z(P), z(P)
    with pytest.raises(RuntimeError, match=r"eval_scores: label_pool must be a contiguous torch.float32"):
        ops.eval_scores(lg, lab.long(), cw, cur, pr, ls)
    with pytest.raises(RuntimeError, match=r"eval_scores: logits must be \(B, 1\)"):
        ops.eval_scores(z(B, 4), lab, cw, cur, pr, ls)
    with pytest.raises(RuntimeError, match=r"eval_scores: clip_w must be .*shape \(4,\)"):
        ops.eval_scores(lg, lab, z(B + 1), cur, pr, ls)
    with pytest.raises(RuntimeError, match=r"eval_scores: cursor must be a contiguous torch.int64"):
        ops.eval_scores(lg, lab, cw, z(1, dtype=torch.int32), pr, ls)
    with pytest.raises(RuntimeError, match=r"eval_scores: losses must be .*shape \(23,\)"):
        ops.eval_scores(lg, lab, cw, cur, pr, z(P - 1))
    with pytest.raises(RuntimeError, match=r"eval_scores: rank=2 of world=2"):
        ops.eval_scores(lg, lab, cw, cur, pr, ls, 2, 2)
    with pytest.raises(RuntimeError, match=r"eval_metrics: labels must be a contiguous torch.int64"):
        ops.eval_metrics(z(P, 4), lab, ls)
    with pytest.raises(RuntimeError, match=r"eval_metrics: probs must be \(P,\)"):
        ops.eval_metrics(z(P, 1), lab, ls)
    with pytest.raises(RuntimeError, match=rf"P={big} clips exceed the limit"):
        ops.eval_metrics(z(big), z(big), z(big), ws=z(1, dtype=torch.int32), record=z(16, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"eval_metrics: ws must be a contiguous int32 vector of at least"):
        ops.eval_metrics(pr, lab, ls, ws=z(3, dtype=torch.int32), record=z(16, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"eval_metrics: record must be .*shape \(16,\)"):
        ops.eval_metrics(pr, lab, ls, ws=ops.eval_metrics_buffers(P, 1, device)[0], record=z(15, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"thresh is NaN"):
        ops.eval_metrics(pr, lab, ls, thresh=float("nan"))
    if device != "cpu":
        with pytest.raises(RuntimeError):
            ops.eval_metrics(pr, lab.cpu(), ls)
    # C ABI
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    refused(lib.query("eeg_dcrnn_eval_scores", None, p(lab), 4, p(cw), p(cur), B, 1, 0, 1, P, p(pr), p(ls), None), "null logits")
    refused(lib.query("eeg_dcrnn_eval_scores", p(lg), p(lab), 4, p(cw), p(cur), B, 1, 0, 1, P, None, p(ls), None), "null probs")
    refused(lib.query("eeg_dcrnn_eval_scores", p(lg), p(lab), 8, p(cw), p(cur), B, 1, 0, 1, P, p(pr), p(ls), None), "label_bytes=8")
    refused(lib.query("eeg_dcrnn_eval_scores", p(lg), p(lab), 4, p(cw), p(cur), B, 1, 0, 1, big, p(pr), p(ls), None), f"P={big}")
    refused(lib.query("eeg_dcrnn_eval_scores", p(lg), p(lab), 4, p(cw), p(cur), B, 1, 1, 1, P, p(pr), p(ls), None), "rank=1 of world=1")
    rec = z(16, dtype=torch.int64)
    refused(lib.query("eeg_dcrnn_eval_metrics", p(pr), p(lab), 4, p(ls), P, 1, 0, 0.5, None, p(rec), None), "null workspace")
    refused(lib.query("eeg_dcrnn_eval_metrics", p(pr), p(lab), 4, p(ls), big, 1, 0, 0.5, p(pr), p(rec), None), f"P={big}")
    refused(lib.query("eeg_dcrnn_eval_metrics", p(pr), p(lab), 4, p(ls), P, 4, 0, 0.5, None, p(rec), None), "label_bytes=4")
    refused(lib.query("eeg_dcrnn_eval_metrics", p(pr), p(lab), 4, p(ls), P, 1, 0, 0.5, p(pr), None, None), "null probs / labels / losses / record")
    assert lib.query("eeg_dcrnn_eval_metrics_ws_bytes", big, 1) == 0 and lib.query("eeg_dcrnn_eval_metrics_ws_bytes", 0, 1) == 0
    assert lib.query("eeg_dcrnn_eval_metrics_ws_bytes", 23, 1) == 4 * 32 + 4 * 33 and lib.query("eeg_dcrnn_eval_metrics_ws_bytes", 23, 4) == 0
    assert bool((pr == 0).all()) and bool((ls == 0).all()) and bool((rec == 0).all())      # no refused call wrote anything


def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on both operators"""
    from eeg_gnn_ssl_amd import ops
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    d = lambda t: t.to(device)     # noqa: E731
    cw = d(torch.tensor([1.0, 1.0, 0.0, 1.0]))
    cur = d(torch.tensor([8], dtype=torch.int64))
    samples = [
        (E.eval_scores.default, (d(torch.randn(B, 1, generator=g)), d(torch.rand(P, generator=g).round()), cw, cur, 0, 1, d(torch.zeros(P)), d(torch.zeros(P)))),
        (E.eval_scores.default, (d(torch.randn(B, 4, generator=g)), d(torch.randint(0, 4, (P,), generator=g)), cw, cur, 1, 2, d(torch.zeros(P, 4)),
                                 d(torch.zeros(P)))),
        (E.eval_metrics.default, (d(torch.rand(P, generator=g)), d(torch.rand(P, generator=g).round()), d(torch.rand(P, generator=g)), True, 0.5,
                                  *ops.eval_metrics_buffers(P, 1, device))),
        (E.eval_metrics.default, (d(torch.softmax(torch.randn(P, 4, generator=g), 1)), d(torch.randint(0, 4, (P,), generator=g)),
                                  d(torch.rand(P, generator=g)), False, 0.5, *ops.eval_metrics_buffers(P, 4, device))),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
