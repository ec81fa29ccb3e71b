"""Checks of the SSL evaluation pass on the device (eeg_gnn_ssl_amd/evaluation.py: `DeviceSSLEvaluator`, csrc/kernels_eval.h): the
per-clip masked-MAE kernel (`ops.ssl_eval_scores`) against a numpy restatement, its independence of where a clip sits, the pass's
record (`ops.ssl_eval_metrics`) against float64 numpy, `TrainStep.ssl_evaluator` against the unchanged `evaluate_ssl` and against the
reference's arithmetic on the host, the pools `evaluate_ssl` cannot be handed (raw pairs, time-domain pairs), the absence of side
effects, the captured pass, and refusals.  As in eval_pass_suite.py the same functions run on the GPU library and on the emulator
build of the same kernel sources (tests/test_ssl_eval.py).

Each check FAILS ON THE PARENT COMMIT: `ops.ssl_eval_scores`, `ops.ssl_eval_metrics` and `TrainStep.ssl_evaluator` do not exist there."""
import random

import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import assert_close, load, make_args

P, B, T, TY, D, W, N = 11, 4, 4, 3, 8, 200, 19
# the scaler of every check: the inverse transform of a target of 1.5 is 1.5 * 2 - 3 = 0 EXACTLY, so the mask (ys != 0) bites
MEAN, STD, MASKED = -3.0, 2.0, 1.5
SUM_RTOL = 1e-12                  # float64 sums of at most 45 600 non-negative terms that differ in order only: 45 600 * 2^-53 = 5e-12 is the
#                                   worst case of a serial sum, a tree of 256 partial sums of 45 terms each stays below (45 + 8) * 2^-53 = 6e-15
# The pass against `evaluate_ssl`: both take the same float32 |d| per element; evaluate_ssl sums them in float32 -- per thread at
# most 2 pieces of 4 terms at these shapes (a batch holds 4 * 3 * 19 * 200 = 45 600 elements at most: 11 400 pieces over the grid),
# an LDS tree of depth 8, a second stage of at most 4 terms per thread and a tree of depth 8: at most 8 + 8 + 4 + 8 = 28 roundings
# of 2^-24 = 1.7e-6 relative, one more for the division and one for the product with the batch size.  The bound of the issue, 2e-5,
# covers it twelve times over and is kept as it is set.
LOSS_RTOL = 2e-5


def _near(a, b, rtol):
    return abs(a - b) <= rtol * abs(b)


# ---- 1. the scores kernel -------------------------------------------------------------------------------------------------------------
def _clips(count, shape, g, scaled, full_mask=None, broken=None):
    """`count` (pred, target) clips of `shape`: one target in twelve is 1.5 and one in twelve is 0 (masked with / without the scaler);
    clip `full_mask` is masked everywhere, clip `broken` predicts a NaN in its first piece and an Inf in its last element"""
    pred, target = torch.randn((count,) + shape, generator=g), torch.randn((count,) + shape, generator=g)
    pick = torch.randint(0, 12, target.shape, generator=g)
    target[pick == 0], target[pick == 1] = MASKED, 0.0
    if full_mask is not None:
        target[full_mask] = MASKED if scaled else 0.0
    if broken is not None:
        flat_p, flat_t = pred[broken].view(-1), target[broken].view(-1)
        flat_p[3], flat_p[-1] = float("nan"), float("inf")
        flat_t[3], flat_t[-1] = 0.7, -0.4
    return pred, target


def restate_clip(pred, target, scaled, mask_val=0.0):
    """numpy: float32 `p * std` then `+ mean` (two roundings), float32 |d|, mask ys != mask_val, float64 sum -> (abs_sum, count, bad)"""
    p, y = pred.numpy().astype(np.float32).reshape(-1), target.numpy().astype(np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        if scaled:
            p = (p * np.float32(STD)).astype(np.float32) + np.float32(MEAN)
            y = (y * np.float32(STD)).astype(np.float32) + np.float32(MEAN)
        d = (p - y).astype(np.float32)
    mk, fin = y != np.float32(mask_val), np.isfinite(d)
    return float(np.abs(d[mk & fin]).astype(np.float64).sum()), float(mk.sum()), float((mk & ~fin).sum())


def _scaler(scaled):
    return dict(mean=MEAN, std=STD) if scaled else dict()


def check_scores_kernel(device):
    """`ops.ssl_eval_scores` on clips of 76 (Ty = 1, N = 19, D = 4: fewer pieces than a workgroup has threads), 5 700 and 45 600
    elements, with and without the scaler: B = 5 slots with clip_w = [1, 1, 1, 0, 1]; slot 1 is masked everywhere, slot 2 predicts a
    NaN and an Inf.  Pool of 3 with the batch at -1 (slot 0 below 0, slot 4 at P: both refused by the kernel's own bound, their weight
    is 1); pool of 7 with the batch at 0, across the end, behind it, far away and at the other end of int64; ranks (0, 1) and (1, 2).
    Addressed positions: count and bad exact, abs_sum within 1e-12 of the restatement, keep bit for bit; every other position keeps
    the sentinel, and so do the rows around the buffers."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(5)
    b, sentinel = 5, -7.0
    clip_w = torch.tensor([1.0, 1.0, 1.0, 0.0, 1.0])
    cases = 0
    for shape in ((1, N, 4), (3, N, 100), (12, N, 200)):
        for scaled in (True, False):
            pred, target = _clips(b, shape, g, scaled, full_mask=1, broken=2)
            want = [restate_clip(pred[s], target[s], scaled) for s in range(b)]
            assert want[1] == (0.0, 0.0, 0.0) and want[2][2] == 2.0 and want[0][1] < pred[0].numel() and want[0][2] == 0.0
            pd, td, wd = pred.to(device), target.to(device), clip_w.to(device)
            for pool, starts in ((3, (-1,)), (7, (0, 5, 7, 2 ** 62 + 5, -2 ** 63 + 3))):
                for rank, world in ((0, 1), (1, 2)):
                    for c0 in starts:
                        if shape[0] == 12 and (c0 > 7 or c0 < -1):
                            continue                                  # (the far cursors write nothing: the two small shapes show it)
                        cursor = (torch.tensor([c0], dtype=torch.int64) + b * world).to(device)     # (wraps like the device's int64 would)
                        sbuf = torch.full((5, pool), sentinel, dtype=torch.float64, device=device)
                        kbuf = torch.full((pool + 2,) + shape, sentinel, dtype=torch.float32, device=device)
                        scores, keep = sbuf[1:4], kbuf[1:-1]
                        ops.ssl_eval_scores(pd, td, wd, cursor, scores, rank, world, keep=keep, **_scaler(scaled))
                        tag = (shape, scaled, pool, rank, world, c0)
                        assert bool((sbuf[0] == sentinel).all()) and bool((sbuf[4] == sentinel).all()), tag
                        assert bool((kbuf[0] == sentinel).all()) and bool((kbuf[-1] == sentinel).all()), tag
                        written = {}
                        for slot in range(b):
                            pos = c0 + rank * b + slot
                            if clip_w[slot] != 0 and 0 <= pos < pool:
                                written[pos] = slot
                        got, kept = scores.cpu(), keep.cpu()
                        for pos in range(pool):
                            if pos not in written:
                                assert bool((got[:, pos] == sentinel).all()) and bool((kept[pos] == sentinel).all()), (tag, pos)
                                continue
                            s = written[pos]
                            a, c, bad = (float(v) for v in got[:, pos])
                            assert (c, bad) == want[s][1:], (tag, pos, c, bad, want[s])
                            assert abs(a - want[s][0]) <= SUM_RTOL * want[s][0], (tag, pos, a, want[s][0])
                            assert torch.equal(kept[pos].view(torch.int32), pred[s].view(torch.int32)), (tag, pos)
                            cases += 1
    assert cases == 6 * (2 + 4 + 2 + 2)      # per shape and scaler: the pool of 3 (2), the pool of 7 at 0 (4) and across its end (2), rank 1 (2)


# ---- 2. placement independence ----------------------------------------------------------------------------------------------------------
def _run_pool(ops, pred, target, b, device, world=1, shift=0, scaled=True):
    """the 11 clips through batches of `b` slots per rank: step k takes the clips (shift + k * b * world + ..) mod 11 as the gather
    would, every rank's launch writes the one buffer -> scores (3, 11)"""
    count = pred.shape[0]
    scores = torch.zeros(3, count, dtype=torch.float64, device=device)
    c0 = shift
    for _ in range(-(-(count - shift) // (b * world))):
        for rank in range(world):
            pos = torch.arange(b) + c0 + rank * b
            valid = (pos >= 0) & (pos < count)
            idx = pos % count
            cursor = torch.tensor([c0 + b * world], dtype=torch.int64, device=device)
            ops.ssl_eval_scores(pred[idx].contiguous().to(device), target[idx].contiguous().to(device), valid.float().to(device), cursor, scores,
                                rank, world, **_scaler(scaled))
        c0 += b * world
    return scores


def check_placement_independence(device):
    """the same 11 clips of 5 700 elements through B = 11 (one launch), B = 4, B = 5, B = 4 on two ranks, and B = 4 with the first
    batch at -1 and at -3 (every clip lands in another slot): the (3, 11) buffers are bitwise equal; a second run of the same
    launches is bitwise equal; and so it is without the scaler"""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(17)
    for scaled in (True, False):
        pred, target = _clips(P, (3, N, 100), g, scaled, full_mask=6)
        base = _run_pool(ops, pred, target, P, device, scaled=scaled)
        want = np.array([restate_clip(pred[i], target[i], scaled) for i in range(P)]).T
        assert np.array_equal(base.cpu().numpy()[1:], want[1:]) and float(base[1].min()) == 0.0
        np.testing.assert_allclose(base.cpu().numpy()[0], want[0], rtol=SUM_RTOL, atol=0)
        for b, world, shift in ((4, 1, 0), (5, 1, 0), (4, 2, 0), (4, 1, -1), (4, 1, -3), (P, 1, 0), (4, 1, 0)):
            again = _run_pool(ops, pred, target, b, device, world, shift, scaled)
            assert torch.equal(base.view(torch.int64), again.view(torch.int64)), (scaled, b, world, shift)


# ---- 3. the record ----------------------------------------------------------------------------------------------------------------------
def restate_record(scores, group):
    """float64 numpy: the words of the record by name"""
    a, c, bad = (np.asarray(v, dtype=np.float64) for v in scores)
    p, loss, empty, batches = len(a), 0.0, 0, 0
    for lo in range(0, p, group):
        hi = min(lo + group, p)
        sg, cg = a[lo:hi].sum(), c[lo:hi].sum()
        loss += (hi - lo) * (sg / cg if cg > 0 else 0.0)
        empty += cg == 0
        batches += 1
    return {"n": p, "batches": batches, "loss": loss / p, "pool_mae": a.sum() / c.sum() if c.sum() > 0 else 0.0, "abs_sum": a.sum(),
            "count": c.sum(), "bad": bad.sum(), "empty_batches": empty}


def check_record(device):
    """`ops.ssl_eval_metrics` against float64 numpy within 1e-12: P = 11 with G = 4 (groups of 4, 4, 3), 11, 1 and 20 (above P: one
    group); the second group masked everywhere (it counts 0 with its weight, empty_batches = 1); everything masked (loss = pool_mae
    = 0, no NaN); P = 700 with G = 255, 256 and 300 (from 256 on the block sums one group after the other) and P = 5000 with G = 7;
    two runs give the same bits"""
    from eeg_gnn_ssl_amd import ops
    rng = np.random.default_rng(3)
    cases = []
    for p, groups in ((11, (4, 11, 1, 20)), (700, (255, 256, 300)), (5000, (7,))):
        a, c = rng.random(p) * 500.0, rng.integers(1, 45600, p).astype(np.float64)
        zero = rng.random(p) < 0.1
        a[zero], c[zero] = 0.0, 0.0
        bad = np.zeros(p)
        bad[p // 2] = 3.0
        cases += [((a, c, bad), g) for g in groups]
    a, c = rng.random(11) * 9.0, rng.integers(1, 99, 11).astype(np.float64)
    a[4:8], c[4:8] = 0.0, 0.0
    cases += [((a, c, np.zeros(11)), 4), ((np.zeros(11), np.zeros(11), np.zeros(11)), 4), ((np.zeros(700), np.zeros(700), np.zeros(700)), 300)]
    for scores, group in cases:
        dev = torch.tensor(np.stack(scores), dtype=torch.float64, device=device)
        rec = ops.ssl_eval_metrics(dev, group).cpu()
        got, want = dict(zip(ops.SSL_EVAL_RECORD, rec.tolist())), restate_record(scores, group)
        assert list(got) == ["n", "batches", "loss", "pool_mae", "abs_sum", "count", "bad", "empty_batches"]
        for k, v in want.items():
            assert np.isfinite(got[k]) and abs(got[k] - v) <= 1e-12 * abs(v), (len(scores[0]), group, k, got[k], v)
        assert torch.equal(rec, ops.ssl_eval_metrics(dev, group, torch.full((8,), -1.0, dtype=torch.float64, device=device)).cpu())
    masked_group = restate_record(cases[-3][0], 4)
    assert masked_group["empty_batches"] == 1 and masked_group["batches"] == 3 and masked_group["loss"] > 0
    assert restate_record(cases[-2][0], 4)["loss"] == 0.0 and restate_record(cases[-2][0], 4)["empty_batches"] == 3


# ---- 4. / 5. the pass -------------------------------------------------------------------------------------------------------------------
RAW_MEAN, RAW_STD = 4.1, 1.6       # the featurisation's z-score of the raw pools


def _case(kind, adj3d, device, units, clips=P, dropout=0.0, curriculum=False):
    """-> (model, TrainStep keywords, dataset, supports, hand() -> the (x, y, supports) batches of B clips for `evaluate_ssl`)
    kind: "shared" (features, the shared distance graph), "corr" (features, supports=None), "raw_fft" (raw pair, raw_window = 200),
    "time_domain" (raw pair, use_fft=False: D = 200)"""
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, DeviceDataset, ops, utils
    g = torch.Generator().manual_seed(41)
    d = {"shared": D, "corr": D, "raw_fft": W // 2, "time_domain": W}[kind]
    cfg = orc.DCRNNConfig(filter_type="laplacian" if kind == "shared" else "dual_random_walk", input_dim=d, output_dim=d, rnn_units=units)
    spans = [(i, min(i + B, clips)) for i in range(0, clips, B)]
    if kind in ("shared", "corr"):
        x = torch.randn(clips, T, N, d, generator=g)
        y = torch.randn(clips, TY, N, d, generator=g)
        y[torch.randint(0, 12, y.shape, generator=g) == 0] = MASKED
        x, y = x.to(device), y.to(device)
        supports = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")] if kind == "shared" else None
        kw = dict(scaler_mean=MEAN, scaler_std=STD)
        hand = lambda: [(x[i:j], y[i:j], supports) for i, j in spans]     # noqa: E731
    else:
        x, y = (20.0 * torch.randn(clips, N, T * W, generator=g)).to(device), (20.0 * torch.randn(clips, N, TY * W, generator=g)).to(device)
        supports = None
        kw = dict(raw_window=W, raw_mean=RAW_MEAN, raw_std=RAW_STD, scaler_mean=RAW_MEAN, scaler_std=RAW_STD, use_fft=kind == "raw_fft")

        def hand():
            if kind == "raw_fft":
                plain, xf, yf = ops.fft_features_pair(x, y, window=W, mean=RAW_MEAN, std=RAW_STD)
                return [(xf[i:j], yf[i:j], ops.correlation_supports(plain[i:j], top_k=3)) for i, j in spans]
            xf, yf = ops.window_features_pair(x, y, W, RAW_MEAN, RAW_STD)
            return [(xf[i:j], yf[i:j], ops.correlation_supports_raw(x[i:j], top_k=3, window=W)) for i, j in spans]
    args = make_args(cfg)
    args.dropout, args.use_curriculum_learning = dropout, curriculum
    model = DCRNNModel_nextTimePred(args, device=device)
    load(model, orc.init_params(cfg, "ssl", seed=6), device)
    return model, kw, DeviceDataset(x, y), supports, hand


def _reference_on_the_host(pred, target, mean, std):
    """train_ssl.py:255-276 restated on the CPU: per batch of B clips `utils.compute_regression_loss(loss_fn="mae")` with the
    StandardScaler (the host path: float32 torch on CPU tensors), averaged weighted by the batch size"""
    from eeg_gnn_ssl_amd import utils
    sc = utils.StandardScaler(mean, std)
    tot, p = 0.0, pred.shape[0]
    for i in range(0, p, B):
        loss = utils.compute_regression_loss(y_true=target[i:i + B].cpu(), y_predicted=pred[i:i + B].cpu(), standard_scaler=sc, loss_fn="mae",
                                             is_tensor=False)
        tot += float(loss) * (min(i + B, p) - i)
    return tot / p


def check_pass(device, adj3d, kind, units):
    """kind "shared" (the distance graph) / "corr" (supports=None), a feature pool of P = 11, B = 4, Ty = 3: `run(capture=False)`
    against `evaluate_ssl(model, ds.batches(4, supports), mean, std)` and against the reference's arithmetic on the host over the
    kept predictions, both within 2e-5 (LOSS_RTOL above); the kept predictions against `evaluate_ssl(return_predictions=True)` --
    bit for bit on the GPU library, at parity_suite's tolerance on the emulator; the record's words; `loss_batch`"""
    from eeg_gnn_ssl_amd.train_step import TrainStep, evaluate_ssl
    model, kw, ds, supports, _ = _case(kind, adj3d, device, units)
    model.train()
    st = TrainStep(model, task="ssl", **kw)
    ev = st.ssl_evaluator(ds, B, supports=supports, keep_predictions=True)
    got = ev.run(capture=False)
    assert model.training and st.sampler is None and ev.sampler.steps_per_epoch == 3 and int(ev.sampler.cursor.item()) == 3 * B
    want, preds, truths = evaluate_ssl(model, ds.batches(B, supports), MEAN, STD, return_predictions=True)
    host = _reference_on_the_host(ev.predictions, ds.y, MEAN, STD)
    print(f"ssl pass {kind}: device {got!r}, evaluate_ssl {want!r} (rel {abs(got - want) / want:.2e}), host reference {host!r} "
          f"(rel {abs(got - host) / host:.2e})")
    assert _near(got, want, LOSS_RTOL) and _near(got, host, LOSS_RTOL), (kind, got, want, host)
    if device == "cpu":
        assert_close(ev.predictions.cpu().numpy(), preds, f"ssl pass {kind}: predictions")
    else:
        assert np.array_equal(ev.predictions.cpu().numpy(), preds), f"ssl pass {kind}: predictions differ by " \
            f"{np.abs(ev.predictions.cpu().numpy() - preds).max():.3e}"
    assert np.array_equal(truths, ds.y.cpu().numpy())
    res = ev.result
    counted = float(((ds.y * STD + MEAN) != 0).sum())
    assert list(res) == ["n", "batches", "loss", "pool_mae", "abs_sum", "count", "bad", "empty_batches"] and res["loss"] == got
    assert (res["n"], res["batches"], res["count"], res["bad"], res["empty_batches"]) == (P, 3, counted, 0, 0) and counted < ds.y.numel()
    clips = np.array([restate_clip(ev.predictions[i].cpu(), ds.y[i].cpu(), True) for i in range(P)]).T
    assert np.array_equal(ev.clip_count.cpu().numpy(), clips[1])
    np.testing.assert_allclose(ev.clip_abs.cpu().numpy(), clips[0], rtol=SUM_RTOL, atol=0)
    np.testing.assert_allclose(ev.clip_mae.cpu().numpy(), clips[0] / clips[1], rtol=2 * SUM_RTOL, atol=0)
    assert _near(res["pool_mae"], clips[0].sum() / clips[1].sum(), SUM_RTOL)
    # loss_batch: the batch size of the loss is independent of the batch size of the pass
    whole = st.ssl_evaluator(ds, B, supports=supports, loss_batch=P)
    assert _near(whole.run(capture=False), res["pool_mae"], SUM_RTOL) and whole.result["batches"] == 1 and whole.predictions is None
    assert torch.equal(whole._scores, ev._scores)


def check_new_ground(device, adj3d, kind, units):
    """what `evaluate_ssl` cannot be handed directly: kind "raw_fft" (raw input (P, 19, 4 * 200) and raw target (P, 19, 3 * 200),
    raw_window = 200, supports=None) and "time_domain" (use_fft=False: D = 200).  The pass equals `evaluate_ssl` on the features /
    windows that `ops.fft_features_pair` / `ops.window_features_pair` give for the whole pool, with the graph of the plain input
    clip, within 2e-5"""
    from eeg_gnn_ssl_amd.train_step import TrainStep, evaluate_ssl
    model, kw, ds, supports, hand = _case(kind, adj3d, device, units)
    st = TrainStep(model, task="ssl", **kw)
    ev = st.ssl_evaluator(ds, B, supports=None)
    got = ev.run(capture=False)
    want = evaluate_ssl(model, hand(), RAW_MEAN, RAW_STD)
    print(f"ssl pass {kind}: device {got!r}, evaluate_ssl {want!r} (rel {abs(got - want) / want:.2e})")
    assert np.isfinite(got) and got > 0 and _near(got, want, LOSS_RTOL), (kind, got, want)
    assert ev.result["count"] == P * TY * N * (W // 2 if kind == "raw_fft" else W) and ev.result["batches"] == 3


# ---- 6. no side effects -------------------------------------------------------------------------------------------------------------------
def check_no_side_effects(device, adj3d, units):
    """a `TrainStep(task="ssl", data_augment=True)` over a model with dropout and curriculum learning in train mode, one training
    step taken (a training sampler attached, Adam moments non-zero): after `run`, model.training, step_count / samples_seen and
    their device mirrors, the parameters, exp_avg*, the augmentation and dropout / curriculum Philox states, the host's `random`
    state and the training sampler (object, epoch and cursor) are what they were; the value equals that of a step without
    augmentation, dropout or curriculum over the same parameters"""
    from eeg_gnn_ssl_amd import EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    noisy, kw, ds, supports, _ = _case("shared", adj3d, device, units, dropout=0.5, curriculum=True)
    noisy.train()
    torch.manual_seed(3)
    st = TrainStep(noisy, task="ssl", data_augment=True, feature_std=1.7, **kw)
    train_sampler = EpochSampler(P, B, 77, 0, 1, device=device)
    st.begin_epoch(0, 2, sampler=train_sampler)
    st.step_from(ds, train_sampler, supports)
    ev = st.ssl_evaluator(ds, B, supports=supports)

    def state():
        return (noisy.training, st.step_count, st.samples_seen, st.step_dev.clone(), st.samples_seen_dev.clone(), st.fp.flat.detach().clone(),
                st.exp_avg.clone(), st.exp_avg_sq.clone(), st._augment_rng.clone(), noisy.decoder._dropout_rng.clone(), random.getstate(),
                train_sampler.cursor.clone(), train_sampler._host_cursor, train_sampler.epoch, id(st.sampler), st.lr)

    before = state()
    assert bool(st.exp_avg.abs().sum() > 0) and int(train_sampler.cursor.item()) == B and noisy.training and st.samples_seen == B
    got = ev.run(capture=False)
    for u, v in zip(before, state()):
        assert torch.equal(u, v) if torch.is_tensor(u) else u == v
    assert st.sampler is train_sampler
    plain, kw2, _, _, _ = _case("shared", adj3d, device, units)
    plain.load_state_dict(noisy.state_dict())
    plain.to(device)
    ev2 = TrainStep(plain, task="ssl", **kw2).ssl_evaluator(ds, B, supports=supports)
    assert ev2.run(capture=False) == got and torch.equal(ev._scores, ev2._scores) and torch.equal(ev.record, ev2.record)


# ---- 7. two ranks ---------------------------------------------------------------------------------------------------------------------------
def two_rank_case(adj3d, clips, device="cpu"):
    """(TrainStep, dataset of `clips` clips, supports) of the two-rank check: built alike in every process"""
    from eeg_gnn_ssl_amd.train_step import TrainStep
    model, kw, ds, supports, _ = _case("shared", adj3d, device, 16, clips=clips)
    return TrainStep(model, task="ssl", **kw), ds, supports


# ---- 8. the captured pass (GPU only) ----------------------------------------------------------------------------------------------------
def check_captured(device, adj3d):
    """the captured pass equals the eager pass bit for bit (scores, kept predictions, record, value); after one training step
    between two passes the REPLAYED graph gives another value and equals a fresh eager pass (the parameters are read in place)"""
    from eeg_gnn_ssl_amd import EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    for kind in ("shared", "raw_fft"):
        model, kw, ds, supports, _ = _case(kind, adj3d, device, 64)
        st = TrainStep(model, task="ssl", **kw)
        model.train()
        eager, graph = (st.ssl_evaluator(ds, B, supports=supports, keep_predictions=True) for _ in range(2))
        v_e, v_g = eager.run(capture=False), graph.run(capture=True)
        assert v_e == v_g and torch.equal(eager._scores, graph._scores) and torch.equal(eager.record, graph.record), kind
        assert torch.equal(eager.predictions, graph.predictions) and model.training
        first, handle = graph._scores.clone(), graph._graph
        sampler = EpochSampler(P, B, 5, 0, 1, device=device)
        st.begin_epoch(0, 2, sampler=sampler)
        st.step_from(ds, sampler, supports)                          # the parameters move
        v_g2 = graph.run(capture=True)
        assert graph._graph is handle and v_g2 != v_g and not torch.equal(first, graph._scores), kind
        fresh = st.ssl_evaluator(ds, B, supports=supports, keep_predictions=True)
        assert fresh.run(capture=False) == v_g2 and torch.equal(fresh._scores, graph._scores) and torch.equal(fresh.record, graph.record), kind
        assert torch.equal(fresh.predictions, graph.predictions)


def check_captured_beside_training_graph(device, adj3d):
    """a `capture_epoch` graph and the evaluation graph alive together: the training losses of two epochs with a captured pass between
    them equal, bit for bit, those of the same two epochs without"""
    from eeg_gnn_ssl_amd import EpochSampler
    from eeg_gnn_ssl_amd.train_step import TrainStep
    runs = []
    for with_pass in (False, True):
        model, kw, ds, supports, _ = _case("shared", adj3d, device, 64)
        model.train()
        torch.manual_seed(99)
        st = TrainStep(model, task="ssl", **kw)
        sampler = EpochSampler(P, B, 5, 0, 1, device=device)
        sampler.begin_epoch(0)
        keep = st.snapshot()
        st.capture_epoch(ds, sampler, supports, include_update=True)
        st.restore(keep)
        ev = st.ssl_evaluator(ds, B, supports=supports)
        losses = []
        for e in range(2):
            st.begin_epoch(e, 2)
            losses += [st.replay_step().clone() for _ in range(sampler.steps_per_epoch)]
            if with_pass and e == 0:
                assert np.isfinite(ev.run(capture=True)) and int(sampler.cursor.item()) == sampler.steps_per_epoch * B
        runs.append((torch.stack(losses), st.fp.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].unique().numel() == runs[0][0].numel()


# ---- 9. refusals, operator registration ------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d):
    """the evaluator: a task other than ssl (the message names `evaluator`), a label pool, pools on another device, batch_size*world
    > P, P over the limit, a raw target that is not (P, N, Ty*raw_window), an output_dim that is no multiple of 4, capture without
    HIP graphs, a non-finite prediction (ValueError after the pass); `TrainStep.evaluator` still refuses ssl with its own message;
    the operators refuse D % 4 != 0, misaligned views, clips of 2^24 elements, other shapes, dtypes and devices before the call; the
    C entry points refuse null pointers and the same limits; no refused call writes"""
    import ctypes
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, DeviceDataset, _lib, ops, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    model, kw, ds, supports, _ = _case("corr", adj3d, device, 16)
    st = TrainStep(model, task="ssl", **kw)
    with pytest.raises(ValueError, match=r"task='ssl'.*evaluate_ssl"):
        st.evaluator(ds, B)
    det = DCRNNModel_classification(make_args(orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=D, num_classes=1, rnn_units=16)), 1,
                                    device=device).to(device)
    with pytest.raises(ValueError, match=r"task='detection'.*TrainStep\.evaluator"):
        TrainStep(det, task="detection").ssl_evaluator(ds, B)
    with pytest.raises(ValueError, match=r"label pool \(11,\).*TARGET pool"):
        st.ssl_evaluator(DeviceDataset(ds.x, z(P)), B)
    with pytest.raises(ValueError, match=r"DeviceSSLEvaluator: dataset on meta"):
        st.ssl_evaluator(DeviceDataset(torch.zeros(P, T, N, D, device="meta"), torch.zeros(P, TY, N, D, device="meta")), B)
    with pytest.raises(ValueError, match=r"batch_size\*world = 6\*2 clips per step, the pool holds P=11"):
        st.ssl_evaluator(ds, 6, rank=0, world=2)
    big = ops.EVAL_MAX_CLIPS + 1
    with pytest.raises(ValueError, match=rf"P={big} clips, one pass takes at most {ops.EVAL_MAX_CLIPS}"):
        st.ssl_evaluator(DeviceDataset(z(big, 1, 1, 4), z(big, 1, 1, 4)), B)
    with pytest.raises(ValueError, match=r"without raw_window the pools hold features"):
        st.ssl_evaluator(DeviceDataset(z(P, N, T * W), z(P, N, TY * W)), B)
    raw = TrainStep(model, task="ssl", raw_window=W)
    for bad_y in (z(P, N, TY * W + 4), z(P, N + 1, TY * W), z(P, TY, N, D)):
        with pytest.raises(ValueError, match=rf"RAW pools: x \(P, N, T\*{W}\) and the target \(P, N, Ty\*{W}\)"):
            raw.ssl_evaluator(DeviceDataset(z(P, N, T * W), bad_y), B)
    with pytest.raises(ValueError, match=r"loss_batch=0"):
        st.ssl_evaluator(ds, B, loss_batch=0)
    odd = DCRNNModel_nextTimePred(make_args(orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=6, output_dim=6, rnn_units=16)),
                                  device=device).to(device)
    with pytest.raises(ValueError, match=r"output_dim=6 is no multiple of 4.*evaluate_ssl"):
        TrainStep(odd, task="ssl").ssl_evaluator(DeviceDataset(z(P, T, N, 6), z(P, 2, N, 6)), B)      # (rows of whole 16-byte pieces)
    if device == "cpu":
        with pytest.raises(RuntimeError, match=r"DeviceSSLEvaluator\.run\(capture=True\) needs HIP graphs"):
            st.ssl_evaluator(ds, B).run()
    broken = DeviceDataset(ds.x.clone(), ds.y)
    broken.x[5, 0, 0, 0] = float("nan")
    ev = st.ssl_evaluator(broken, B, supports=[s.to(device) for s in utils.compute_supports(adj3d, "dual_random_walk")])
    with pytest.raises(ValueError, match=r"predictions are NaN or infinite where the target counts"):
        ev.run(capture=False)
    assert ev.result["bad"] > 0 and float(ev._scores[2, 5]) > 0 and float(ev._scores[2, :4].sum()) == 0      # (clip 5, its batch at most)
    # the operators
    pr, tg, cw, cur, sc = z(B, TY, N, D), z(B, TY, N, D), z(B), z(1, dtype=torch.int64), z(3, P, dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: pred \(4, 3, 19, 8\) and target \(4, 3, 19, 4\) differ in shape"):
        ops.ssl_eval_scores(pr, z(B, TY, N, 4), cw, cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: D=6: .* multiple of 4"):
        ops.ssl_eval_scores(z(B, TY, N, 6), z(B, TY, N, 6), cw, cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: pred is not 16-byte aligned"):
        ops.ssl_eval_scores(z(B * TY * N * D + 4)[1:-3].view(B, TY, N, D), tg, cw, cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: keep is not 16-byte aligned"):
        ops.ssl_eval_scores(pr, tg, cw, cur, sc, keep=z(P * TY * N * D + 4)[1:-3].view(P, TY, N, D))
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: pred must be a contiguous"):
        ops.ssl_eval_scores(z(TY, B, N, D).transpose(0, 1), tg, cw, cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: a clip of 16777216 elements"):
        ops.ssl_eval_scores(z(1, 1, 1, 1).expand(1, 2 ** 12, 2 ** 10, 4), z(1, 1, 1, 1).expand(1, 2 ** 12, 2 ** 10, 4), z(1), cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: clip_w must be .*shape \(4,\)"):
        ops.ssl_eval_scores(pr, tg, z(B + 1), cur, sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: cursor must be a contiguous torch.int64"):
        ops.ssl_eval_scores(pr, tg, cw, z(1, dtype=torch.int32), sc)
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: scores must be \(3, P\) float64"):
        ops.ssl_eval_scores(pr, tg, cw, cur, z(P, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"scores: expected dtype torch.float64"):
        ops.ssl_eval_scores(pr, tg, cw, cur, z(3, P))
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: keep must be .*shape \(11, 3, 19, 8\)"):
        ops.ssl_eval_scores(pr, tg, cw, cur, sc, keep=z(P - 1, TY, N, D))
    with pytest.raises(RuntimeError, match=r"ssl_eval_scores: rank=2 of world=2"):
        ops.ssl_eval_scores(pr, tg, cw, cur, sc, 2, 2)
    with pytest.raises(RuntimeError, match=r"ssl_eval_metrics: groups of 0 clips"):
        ops.ssl_eval_metrics(sc, 0)
    with pytest.raises(RuntimeError, match=r"ssl_eval_metrics: record must be .*shape \(8,\)"):
        ops.ssl_eval_metrics(sc, 4, z(7, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=rf"P={big} clips exceed the limit"):
        ops.ssl_eval_metrics(z(3, big, dtype=torch.float64), 4)
    if device != "cpu":
        with pytest.raises(RuntimeError):
            ops.ssl_eval_scores(pr, tg.cpu(), cw, cur, sc)
    # C ABI
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    per = TY * N * D

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    def scores_call(pred=p(pr), target=p(tg), b=B, elems=per, d=D, rank=0, world=1, pool=P, scores=p(sc), keep=None):
        return lib.query("eeg_dcrnn_ssl_eval_scores", pred, target, p(cw), p(cur), b, elems, d, rank, world, pool, 1, MEAN, STD, 0.0, scores, keep, None)

    refused(scores_call(pred=None), "null pred")
    refused(scores_call(scores=None), "null scores")
    refused(scores_call(d=6, elems=TY * N * 6), "D=6")
    refused(scores_call(elems=per + 4), "no whole number of rows")
    refused(scores_call(elems=2 ** 24, d=4), "a clip of 16777216 elements")
    refused(scores_call(pool=big), f"P={big}")
    refused(scores_call(rank=1), "rank=1 of world=1")
    refused(scores_call(pred=ctypes.c_void_p(pr.data_ptr() + 4)), "16-byte aligned")
    refused(scores_call(keep=ctypes.c_void_p(pr.data_ptr() + 8)), "16-byte aligned")
    rec = z(8, dtype=torch.float64)
    refused(lib.query("eeg_dcrnn_ssl_eval_metrics", None, P, 4, p(rec), None), "null scores / record")
    refused(lib.query("eeg_dcrnn_ssl_eval_metrics", p(sc), big, 4, p(rec), None), f"P={big}")
    refused(lib.query("eeg_dcrnn_ssl_eval_metrics", p(sc), P, 0, p(rec), None), "G=0")
    assert bool((sc == 0).all()) and bool((rec == 0).all()) and bool((pr == 0).all())      # no refused call wrote anything


def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on both operators"""
    from eeg_gnn_ssl_amd import ops
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    d = lambda t: t.to(device)     # noqa: E731
    cw = d(torch.tensor([1.0, 1.0, 0.0, 1.0]))
    cur = d(torch.tensor([8], dtype=torch.int64))
    pred, target = d(torch.randn(B, TY, N, D, generator=g)), d(torch.randn(B, TY, N, D, generator=g))
    scores, record, keep = ops.ssl_eval_buffers(P, device, (TY, N, D))
    filled = d(torch.rand(3, P, generator=g, dtype=torch.float64))
    samples = [
        (E.ssl_eval_scores.default, (pred, target, cw, cur, 0, 1, True, MEAN, STD, 0.0, scores, None)),
        (E.ssl_eval_scores.default, (pred, target, cw, cur, 1, 2, False, 0.0, 1.0, 0.0, scores, keep)),
        (E.ssl_eval_metrics.default, (filled, 4, record)),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
