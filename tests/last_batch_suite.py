"""Checks of an epoch that keeps its short last batch (`EpochSampler(..., drop_last=False)`, the reference's `DataLoader` default): the
validity gather (`ops.gather_clips(..., clip_w=, denom=, n_valid=)`), the weighted criteria (`ops.cls_head_loss`, `bce_with_logits`,
`cross_entropy`, `masked_regression_loss` with `clip_w=, denom=`), the device increment of `ops.teacher_flags`, and
`TrainStep.step_from` / `capture_epoch` / checkpointing with such a sampler.  As in device_epoch_suite.py the same functions run on
the GPU library and on the emulator build of the same kernel sources (tests/test_last_batch.py); the shapes are that suite's.

Tolerances: `torch.equal` wherever the arithmetic is the same (a full batch through the weighted kernels; whatever sits in a slot
that does not count); `parity_suite.TOL` (2e-5 of the tensor's largest magnitude) where a padded batch of 4 is compared with the
same clips run as a batch of 3 or 7 (other sums, other GEMM shapes), 1e-6 absolute on per-clip gradients of order one (the
tolerance parity_suite uses for the loss kernels' gradients), and 2 * TOL on parameters and moments behind one Adam step.

Each check FAILS ON THE PARENT COMMIT: the `drop_last` argument, the `clip_w` / `denom` / `n_valid` arguments and the entry points
behind them do not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from device_epoch_suite import B, D, P, SEED, T, TY, W, _guarded, _same_state, _state, _step_case
from parity_suite import TOL, assert_close_scaled

N = 19
HEAD_B, HEAD_H = 6, 64            # one full workgroup of four waves and one with two
REG_SHAPE = (5, 2, N, 12)         # 5 clips of 456 elements: no multiple of a block's stretch, blocks straddle clips
HEAD_W = [1., 0., 1., 1., 0., 1.]
REG_W = [1., 1., 0., 1., 0.]


def _f(values, device):
    return torch.tensor(values, dtype=torch.float32, device=device)


# ---- 1. the validity gather ----------------------------------------------------------------------------------------------------------
def check_gather_validity(device):
    """`ops.gather_clips(..., clip_w=, denom=, n_valid=)`: the copies are those of the plain gather (wrap included), the cursor
    advances by B*world, and clip_w / n_valid / denom are, at P = 23, B = 4: world 1, cursors 0 / 20 / 24 -> [1,1,1,1], 4, 4 /
    [1,1,1,0], 3, 3 / [0,0,0,0], 0, 1; world 2, cursor 16 -> rank 0 [1,1,1,1], rank 1 [1,1,1,0], both 7 and 3.5; the same at P = 19
    (a rank with nothing): rank 0 [1,1,1,0], rank 1 [0,0,0,0], both 3 and 1.5.  All outputs sit between sentinel rows."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(41)
    d = lambda t: t.to(device)     # noqa: E731
    x_pool, y_pool = torch.randn(P, T, 4, D, generator=g), torch.randn(P, TY, 4, D, generator=g)
    labels, lens = torch.randint(0, 4, (P,), generator=g), torch.randint(1, T + 1, (P,), generator=g)
    cases = [(P, 0, 1, 0, [1, 1, 1, 1], 4, 4.0), (P, 0, 1, 20, [1, 1, 1, 0], 3, 3.0), (P, 0, 1, 24, [0, 0, 0, 0], 0, 1.0),
             (P, 0, 2, 16, [1, 1, 1, 1], 7, 3.5), (P, 1, 2, 16, [1, 1, 1, 0], 7, 3.5),
             (19, 0, 2, 16, [1, 1, 1, 0], 3, 1.5), (19, 1, 2, 16, [0, 0, 0, 0], 3, 1.5)]
    for p, rank, world, c0, want_w, want_n, want_d in cases:
        perm = d(torch.randperm(p, generator=g))
        pools = [d(t[:p].contiguous()) for t in (x_pool, y_pool, labels, lens)]
        for wide in (False, True):                                  # labels + lengths / the SSL target as second wide tensor
            outs = []
            for tail in (False, True):
                cursor = d(torch.tensor([c0], dtype=torch.int64))
                x_out, x_ok = _guarded((B, T, 4, D), torch.float32, device)
                y_out, y_ok = _guarded((B, TY, 4, D) if wide else (B,), torch.float32 if wide else torch.int64, device)
                n_out, n_ok = _guarded((B,), torch.int64, device)
                kw = dict(y_pool=pools[1], y_out=y_out) if wide else dict(label_pool=pools[2], label_out=y_out, len_pool=pools[3], len_out=n_out)
                if tail:
                    (cw, cw_ok), (dn, dn_ok), (nv, nv_ok) = (_guarded((B,), torch.float32, device), _guarded((1,), torch.float32, device),
                                                             _guarded((1,), torch.int64, device))
                    kw.update(clip_w=cw, denom=dn, n_valid=nv)
                ops.gather_clips(pools[0], x_out, perm, cursor, rank, world, **kw)
                assert int(cursor.item()) == c0 + B * world and x_ok() and y_ok() and n_ok()
                outs.append((x_out.clone(), y_out.clone(), n_out.clone()))
            tag = (p, rank, world, c0, wide)
            assert all(torch.equal(u, v) for u, v in zip(*outs)), tag
            assert cw.tolist() == want_w and int(nv.item()) == want_n and float(dn.item()) == want_d, (tag, cw.tolist(), nv.item(), dn.item())
            assert cw_ok() and dn_ok() and nv_ok(), tag


# ---- 2. / 3. the weighted criteria -----------------------------------------------------------------------------------------------------
def _head_case(c, device, g):
    z = torch.randn(HEAD_B, N, HEAD_H, generator=g).to(device)
    w, bias = (0.3 * torch.randn(c, HEAD_H, generator=g)).to(device), (0.1 * torch.randn(c, generator=g)).to(device)
    y = ((torch.rand(HEAD_B, generator=g) > 0.5).float() if c == 1 else torch.randint(0, c, (HEAD_B,), generator=g)).to(device)
    return z, w, bias, y


def _head(z, w, bias, y, p_drop=0.0, clip_w=None, denom=None):
    """the fused head operator -> dict of everything it writes (a fresh generator state per call: the same dropout masks)"""
    from eeg_gnn_ssl_amd import ops
    E = torch.ops.eeg_dcrnn
    state = torch.tensor([4242, 11], dtype=torch.int64, device=z.device)
    used = ops.rng_take(state, z.numel() // 4) if p_drop > 0 else None
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    kind = 0 if w.shape[0] == 1 else 1
    if clip_w is None:
        loss, logits, arg, dlogits, dz = E.cls_head_loss(z, w, bias, y, kind, p_drop, used, dw, db)
    else:
        loss, logits, arg, dlogits, dz = E.cls_head_loss_w(z, w, bias, y, kind, p_drop, used, clip_w, denom, dw, db)
    return dict(loss=loss, logits=logits, arg=arg, dlogits=dlogits, dz=dz, dW=dw, dbias=db)


def _reg_case(device, g, masked=True):
    pred, y = torch.randn(REG_SHAPE, generator=g), torch.randn(REG_SHAPE, generator=g)
    if masked:
        y[torch.rand(REG_SHAPE, generator=g) < 0.2] = 0.0          # mask_val: these elements do not count
    return pred.to(device), y.to(device)


REG_VARIANTS = [(kind, scaler) for kind in (0, 1) for scaler in ((False, 0.0, 1.0), (True, 0.3, 1.7))]


def check_full_batch_is_unweighted(device):
    """clip_w = 1 and denom = B: every weighted operator equals its unweighted twin bit for bit (`torch.equal`) on everything it
    writes -- the fused head (C = 1 and 4, dropout 0 and 0.5 with the same generator state, B = 6), `bce_logits_w`, `ce_logits_w`
    and `masked_loss_w` (MAE and RMSE, with and without scaler, 5 clips of 456 elements, masked elements among them)."""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(42)
    ones, denom = _f([1.] * HEAD_B, device), _f([float(HEAD_B)], device)
    for c in (1, 4):
        z, w, bias, y = _head_case(c, device, g)
        for p_drop in (0.0, 0.5):
            want, got = _head(z, w, bias, y, p_drop), _head(z, w, bias, y, p_drop, ones, denom)
            for k in want:
                assert torch.equal(got[k], want[k]), (c, p_drop, k)
            assert np.isfinite(float(want["loss"]))
        lg = want["logits"]
        plain, weighted = (E.bce_logits(lg.view(-1), y), E.bce_logits_w(lg.view(-1), y, ones, denom)) if c == 1 else \
                          (E.ce_logits(lg, y), E.ce_logits_w(lg, y, ones, denom))
        assert torch.equal(weighted[0], plain[0]) and torch.equal(weighted[1], plain[1]), c
    pred, y = _reg_case(device, g)
    ones, denom = _f([1.] * REG_SHAPE[0], device), _f([float(REG_SHAPE[0])], device)
    for kind, (scaled, mean, std) in REG_VARIANTS:
        plain = E.masked_loss(pred, y, scaled, mean, std, 0.0, kind)
        weighted = E.masked_loss_w(pred, y, scaled, mean, std, 0.0, kind, ones, denom)
        assert torch.equal(weighted[0], plain[0]) and torch.equal(weighted[1], plain[1]), (kind, scaled)
        assert float(plain[0]) > 0 and bool((plain[1] == 0).any()) == (not scaled)      # (the masked elements: zero gradient)


def check_kept_clips(device):
    """clip_w = [1,0,1,1,0,1] (head, bce, ce) / [1,1,0,1,0] (regression), denom = the number of ones, against the unweighted
    operator on the kept clips alone: per-clip gradients of kept clips within 1e-6, those of the others exactly zero, loss / dW /
    dbias within TOL; logits and arg are those of the whole batch.  A cross-entropy label of -1 on a clip that does not count
    leaves everything as it is; on a kept clip the loss is NaN.  All weights zero: loss 0, gradients 0.  The DDP factor (two
    ranks, denom = 3.5, 4 and 3 ones): for the MAE without masked elements the ranks' dpred, halved, are the 7-clip criterion's
    gradient within TOL and their halved losses sum to its value; for the RMSE value and gradient are the clip-weighted mean of
    the ranks' own losses (a rank's loss is the loss of its shard), checked against the unweighted operator per shard."""
    E = torch.ops.eeg_dcrnn
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(43)
    cpu = lambda t: t.detach().cpu().numpy()     # noqa: E731
    cw = _f(HEAD_W, device)
    keep = cw != 0
    denom = _f([float(keep.sum())], device)
    zeros, one = _f([0.] * HEAD_B, device), _f([1.], device)
    for c in (1, 4):
        z, w, bias, y = _head_case(c, device, g)
        whole, want, got = _head(z, w, bias, y), _head(z[keep], w, bias, y[keep]), _head(z, w, bias, y, 0.0, cw, denom)
        assert torch.equal(got["logits"], whole["logits"]) and torch.equal(got["arg"], whole["arg"])
        for k in ("dlogits", "dz"):
            err = float((got[k][keep] - want[k]).abs().max())
            print(f"head C={c} {k}: kept clips differ by {err:.2e}, largest {float(want[k].abs().max()):.2e}")
            assert err <= 1e-6, (c, k, err)
            assert float(got[k][~keep].abs().max()) == 0.0 and float(want[k].abs().max()) > 0
        for k in ("loss", "dW", "dbias"):
            assert_close_scaled(cpu(got[k]), cpu(want[k]), f"head C={c} {k}")
        none = _head(z, w, bias, y, 0.0, zeros, one)
        assert all(float(none[k].abs().max()) == 0.0 for k in ("loss", "dlogits", "dz", "dW", "dbias")), c
        lg = whole["logits"]
        crit_w, crit, lgk = (E.bce_logits_w, E.bce_logits, lambda t: t.view(-1)) if c == 1 else (E.ce_logits_w, E.ce_logits, lambda t: t)
        (lw, dw_), (lk, dk) = crit_w(lgk(lg), y, cw, denom), crit(lgk(lg[keep]), y[keep])
        assert_close_scaled(cpu(lw), cpu(lk), f"criterion C={c} loss")
        assert float((lgk(dw_.view_as(lg)[keep]) - dk).abs().max()) <= 1e-6 and float(dw_.view_as(lg)[~keep].abs().max()) == 0.0
        lz, dzero = crit_w(lgk(lg), y, zeros, one)
        assert float(lz) == 0.0 and float(dzero.abs().max()) == 0.0
        if c == 4:
            bad = y.clone()
            bad[1] = -1                                                     # a clip that does not count
            off = _head(z, w, bias, bad, 0.0, cw, denom)
            assert all(torch.equal(off[k], got[k]) for k in got) and np.isfinite(float(off["loss"]))
            assert torch.equal(crit_w(lg, bad, cw, denom)[0], lw)
            assert float(ops.cross_entropy(lg, bad, clip_w=cw, denom=denom)) == float(lw)
            bad[0] = -1                                                     # a kept clip: NaN, as the unweighted kernels
            assert bool(torch.isnan(_head(z, w, bias, bad, 0.0, cw, denom)["loss"])) and bool(torch.isnan(crit_w(lg, bad, cw, denom)[0]))
            assert bool(torch.isnan(_head(z, w, bias, bad)["loss"]))
    # the regression loss
    pred, y = _reg_case(device, g)
    cw = _f(REG_W, device)
    keep = cw != 0
    denom = _f([float(keep.sum())], device)
    for kind, (scaled, mean, std) in REG_VARIANTS:
        lw, dp = E.masked_loss_w(pred, y, scaled, mean, std, 0.0, kind, cw, denom)
        lk, dk = E.masked_loss(pred[keep], y[keep], scaled, mean, std, 0.0, kind)
        assert_close_scaled(cpu(lw), cpu(lk), f"masked loss kind={kind} scaled={scaled}")
        # (dpred is of order 1 / count: the 1e-6 of values of order one, relative to the largest entry)
        assert float((dp[keep] - dk).abs().max()) <= 1e-6 * float(dk.abs().max()) and float(dp[~keep].abs().max()) == 0.0
        lz, dzero = E.masked_loss_w(pred, y, scaled, mean, std, 0.0, kind, _f([0.] * 5, device), _f([1.], device))
        assert float(lz) == 0.0 and float(dzero.abs().max()) == 0.0
    # two ranks: 7 clips, rank 0 holds clips 0..3, rank 1 clips 4..6 and a slot that does not count
    pred7, y7 = torch.randn((7,) + REG_SHAPE[1:], generator=g).to(device), torch.randn((7,) + REG_SHAPE[1:], generator=g).to(device)
    junk = torch.randn((1,) + REG_SHAPE[1:], generator=g).to(device)
    shards = [(pred7[:4], y7[:4], _f([1, 1, 1, 1], device), 4), (torch.cat([pred7[4:], junk]), torch.cat([y7[4:], junk]), _f([1, 1, 1, 0], device), 3)]
    half = _f([3.5], device)
    for kind in (0, 1):
        out = [E.masked_loss_w(p_, y_, True, 0.3, 1.7, 0.0, kind, w_, half) for p_, y_, w_, _ in shards]
        loss = (out[0][0] + out[1][0]) / 2
        grad = torch.cat([out[0][1], out[1][1][:3]]) / 2
        assert float(out[1][1][3].abs().max()) == 0.0
        if kind == 0:
            want_l, want_g = E.masked_loss(pred7, y7, True, 0.3, 1.7, 0.0, 0)
        else:
            own = [E.masked_loss(p_[:k], y_[:k], True, 0.3, 1.7, 0.0, 1) for p_, y_, _, k in shards]
            want_l = (4 * own[0][0] + 3 * own[1][0]) / 7
            want_g = torch.cat([4 * own[0][1], 3 * own[1][1]]) / 7
        assert_close_scaled(cpu(loss), cpu(want_l), f"two ranks, kind={kind}: loss")
        assert_close_scaled(cpu(grad), cpu(want_g), f"two ranks, kind={kind}: dpred")


# ---- 4. what sits in a slot that does not count --------------------------------------------------------------------------------------
def _tail_sampler(device, cursor=None, rank=0, world=1, p=P, epoch=0):
    from eeg_gnn_ssl_amd import EpochSampler
    s = EpochSampler(p, B, SEED, rank, world, device=device, drop_last=False).begin_epoch(epoch)
    return s if cursor is None else s.seek(cursor)


def check_invalid_slot_content(device, adj3d, mode, units=64):
    """two data sets equal on the clips of perm[20:23] and different (finite) on clip perm[0] -- input, label / target and length --
    the clip the wrap puts into the fourth slot of the short step: one `step_from` at cursor 20 on twins gives `torch.equal` loss,
    gradient bucket, parameters and Adam moments.  Catches a weight applied to the value but not to a gradient.  detection: the
    spectral path (asserted)."""
    from eeg_gnn_ssl_amd import DeviceDataset, ops
    make, ds, supports = _step_case(mode, adj3d, device, units)
    probe = _tail_sampler(device)
    other = int(probe.perm[0].item())
    assert other not in probe.perm[20:23].tolist()
    g = torch.Generator().manual_seed(44)
    x2, y2 = ds.x.clone(), ds.y.clone()
    x2[other] = (3.0 * torch.randn(ds.x[other].shape, generator=g)).to(device)
    if ds.y_is_target:
        y2[other] = (3.0 * torch.randn(ds.y[other].shape, generator=g)).to(device)
    else:
        y2[other] = (1 - y2[other]) if mode == "detection" else (y2[other] + 1) % 4
    lens2 = None
    if ds.seq_lengths is not None:
        lens2 = ds.seq_lengths.clone()
        lens2[other] = lens2[other] % T + 1
    ds2 = DeviceDataset(x2, y2, lens2)
    before = ops.spectral_layer_calls
    out = []
    for data in (ds, ds2):
        (_, st) = make()
        s = _tail_sampler(device, 20)
        st.set_epoch(0, 4)
        loss = st.step_from(data, s, supports)
        assert s.clip_w.tolist() == [1, 1, 1, 0] and int(s.n_valid.item()) == 3 and st.samples_seen == 3
        out.append((loss.clone(), st.fp.flat_grad.clone()) + _state(st))
    assert np.isfinite(float(out[0][0])) and float(out[0][1].abs().max()) > 0
    for name, u, v in zip(("loss", "flat_grad", "parameters", "exp_avg", "exp_avg_sq"), *out):
        assert torch.equal(u, v), f"{mode}: {name} depends on the clip in the slot that does not count ({float((u - v).abs().max()):.3e})"
    if mode == "detection":
        assert ops.spectral_layer_calls > before, "the shared 2-D graph takes the spectral form"


# ---- 5. the short step is the reference's short batch ---------------------------------------------------------------------------------
def _within(u, v, tol, what):
    scale = max(float(v.abs().max()), 1e-6)
    err = float((u - v).abs().max()) / scale
    print(f"{what}: differs by {err:.3e} of the largest magnitude {scale:.3e} (allowed {tol:.1e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def _hand_step(st, ds, idx, mode, supports):
    lens = torch.full((idx.numel(),), T, dtype=torch.int64, device=idx.device) if ds.seq_lengths is None else ds.seq_lengths[idx]
    return st.step(ds.x[idx], ds.y[idx], None if mode == "ssl" else lens, supports)


def check_short_step(device, adj3d, mode, units=64):
    """a whole epoch with a drop_last=False sampler (steps_per_epoch == 6) against a twin fed `step(pool[idx], ...)` by hand with
    idx = perm[s*B:(s+1)*B] -- 3 clips at the last step.  Steps 0-4: losses, parameters and moments `torch.equal` (the weighted
    path on a full batch IS the unweighted one).  After step 5: loss within TOL, parameters and moments within 2 * TOL of their
    largest magnitude (one Adam step behind gradients that agree to TOL); samples_seen == 23 and step_count == 6 on both, cursor 24.
    ssl runs WITH data_augment: clip b's draw is Philox counter offset + b, so the twin's three draws are the first three of the
    padded step's four (asserted) -- nothing is handed over."""
    make, ds, supports = _step_case(mode, adj3d, device, units)
    (_, a), (_, b) = make(), make()
    sampler = _tail_sampler(device)
    assert sampler.steps_per_epoch == 6 and not sampler.drop_last
    a.set_epoch(0, 4)
    a.attach_sampler(sampler)
    b.set_epoch(0, 4)
    perm = sampler.perm.clone()
    for s in range(sampler.steps_per_epoch):
        la = a.step_from(ds, sampler, supports)
        lb = _hand_step(b, ds, perm[s * B:(s + 1) * B], mode, supports)
        if s < 5:
            assert torch.equal(la, lb), (mode, s, la.item(), lb.item())
            _same_state(a, b, f"{mode}, step {s}")
            assert sampler.clip_w.tolist() == [1, 1, 1, 1] and float(sampler.denom.item()) == B and a.samples_seen == (s + 1) * B
    assert sampler.clip_w.tolist() == [1, 1, 1, 0] and float(sampler.denom.item()) == 3.0
    _within(la.reshape(1), lb.reshape(1), TOL, f"short step {mode}: loss")
    for name, u, v in zip(("parameters", "exp_avg", "exp_avg_sq"), _state(a), _state(b)):
        _within(u, v, 2 * TOL, f"short step {mode}: {name}")
    assert a.samples_seen == b.samples_seen == P and a.step_count == b.step_count == 6
    assert int(sampler.cursor.item()) == 24 and sampler._host_cursor == 24
    if mode == "ssl":
        for u, v in zip(a.last_augmentation, b.last_augmentation):
            assert torch.equal(u[:3], v)


# ---- 6. two ranks on one device --------------------------------------------------------------------------------------------------------
def check_two_ranks(device, adj3d, units=64):
    """samplers with explicit (rank, world) = (0, 2), (1, 2), `forward_backward` on the last step of the epoch (cursor 16): the mean
    of the two gradient buckets -- the summed all-reduce and its 1/world -- is the gradient of the hand-fed batch of the clips that
    remain, within TOL, and so is the mean of the losses.  P = 23: 4 + 3 clips.  P = 19: 3 + 0 clips -- the gradient of the rank
    with nothing is exactly zero and its loss 0.  Detection mode."""
    from eeg_gnn_ssl_amd import DeviceDataset
    make, ds, supports = _step_case("detection", adj3d, device, units)
    cpu = lambda t: t.detach().cpu().numpy()     # noqa: E731
    for p in (P, 19):
        data = ds if p == P else DeviceDataset(ds.x[:p].contiguous(), ds.y[:p].contiguous())
        grads, losses = [], []
        for rank in (0, 1):
            (_, st) = make()
            s = _tail_sampler(device, 16, rank, 2, p)
            batch = st._epoch_batch(data, s)
            st._gather_batch(data, s, batch)
            losses.append(st.forward_backward(batch[0], batch[1], batch[2], supports, sampler=s).clone())
            grads.append(st.fp.flat_grad.clone())
            assert int(s.n_valid.item()) == p - 16 and float(s.denom.item()) == (p - 16) / 2
        (_, ref) = make()
        idx = s.perm[16:p]
        want_l = ref.forward_backward(data.x[idx], data.y[idx], torch.full((p - 16,), T, dtype=torch.int64, device=device), supports)
        assert_close_scaled(cpu((grads[0] + grads[1]) / 2), cpu(ref.fp.flat_grad), f"two ranks, P={p}: gradient")
        assert_close_scaled(cpu((losses[0] + losses[1]) / 2), cpu(want_l), f"two ranks, P={p}: loss")
        assert float(grads[0].abs().max()) > 0
        if p == 19:
            assert float(grads[1].abs().max()) == 0.0 and float(losses[1]) == 0.0


# ---- 7. the curriculum counter ---------------------------------------------------------------------------------------------------------
def check_curriculum_counter(device):
    """`ops.teacher_flags` with the increment in device memory (int64[1] = 3) equals the call with the host increment 3: flags,
    generator state and counter, over three calls in a row (the threshold decays with the counter)."""
    from eeg_gnn_ssl_amd import ops
    mk = lambda: (torch.tensor([977, 5], dtype=torch.int64, device=device), torch.tensor([40], dtype=torch.int64, device=device))     # noqa: E731
    (st_h, seen_h), (st_d, seen_d) = mk(), mk()
    inc = torch.tensor([3], dtype=torch.int64, device=device)
    for k in range(3):
        host, dev = ops.teacher_flags(st_h, seen_h, 3, 30.0, 6), ops.teacher_flags(st_d, seen_d, inc, 30.0, 6)
        assert torch.equal(host, dev) and host.dtype == torch.int32 and torch.equal(st_h, st_d) and torch.equal(seen_h, seen_d)
        assert int(seen_d.item()) == 40 + 3 * (k + 1) and int(st_d[1].item()) == 5 + 2 * (k + 1)
    assert int(inc.item()) == 3


def check_curriculum_step(device, adj3d):
    """the ssl step with curriculum learning on the device and a drop_last=False sampler: the model's increment is the sampler's
    `n_valid` tensor, so after the full step at cursor 16 and the short one at cursor 20 the device counter and its host mirror
    both stand at 4 + 3; the losses are those of a twin fed the same clips by hand (4, then 3; the same generator states, hence
    the same teacher-forcing flags) within TOL.  Feature pairs of 16 values per node and 64 units: a shape the persistent decoder
    kernels cover (asserted), which is where the flags are drawn on the device."""
    from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, DeviceDataset
    from eeg_gnn_ssl_amd.train_step import TrainStep
    from oracle import dcrnn_oracle as orc
    from parity_suite import load, make_args
    g = torch.Generator().manual_seed(45)
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=16, output_dim=16, rnn_units=64)
    ds = DeviceDataset(torch.randn(P, T, N, 16, generator=g).to(device), torch.randn(P, TY, N, 16, generator=g).to(device))
    params = orc.init_params(cfg, "ssl", seed=6)
    steps = []
    for _ in range(2):
        torch.manual_seed(99)                                      # the seed of the decoder's generator: the same flags on both
        model = DCRNNModel_nextTimePred(make_args(cfg), device=device)
        load(model, params, device)
        model.train()
        model.use_curriculum_learning, model.cl_decay_steps = True, 2.0     # (threshold 0.67 at 0 samples, 0.21 at 4)
        steps.append(TrainStep(model, task="ssl"))
    a, b = steps
    sampler = _tail_sampler(device, 16)
    perm = sampler.perm.clone()
    for lo, hi, seen in ((16, 20, 4), (20, 23, 7)):
        la, lb = a.step_from(ds, sampler, None), _hand_step(b, ds, perm[lo:hi], "ssl", None)
        assert a.device_curriculum and a.model.batches_seen_increment is sampler.n_valid
        assert int(a.samples_seen_dev.item()) == a.samples_seen == seen and int(b.samples_seen_dev.item()) == b.samples_seen == seen
        _within(la.reshape(1), lb.reshape(1), TOL, f"curriculum step at cursor {lo}: loss")
    assert torch.equal(a.model.decoder._dropout_rng, b.model.decoder._dropout_rng) and int(a.model.decoder._dropout_rng[1]) > 0


# ---- 8. resume ---------------------------------------------------------------------------------------------------------------------------
def check_resume(device, adj3d, units=64):
    """`state_dict` after step 4 of a drop_last=False epoch (cursor 20: before the short step), loaded into a fresh TrainStep +
    sampler: the short step gives the parameters of the uninterrupted run, bit for bit; `drop_last` is not in the state, and the
    state of a default sampler is still exactly {seed, epoch, cursor}."""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, supports = _step_case("detection", adj3d, device, units)
    (_, whole) = make()
    s_w = _tail_sampler(device, epoch=1)
    whole.set_epoch(1, 4)
    for _ in range(s_w.steps_per_epoch):
        whole.step_from(ds, s_w, supports)
    (m1, first) = make()
    s_1 = _tail_sampler(device, epoch=1)
    first.set_epoch(1, 4)
    for _ in range(5):
        first.step_from(ds, s_1, supports)
    state, weights = first.state_dict(), {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    assert state["sampler"] == {"seed": SEED, "epoch": 1, "cursor": 5 * B} and state["samples_seen"] == 5 * B
    (m2, second) = make()
    m2.load_state_dict(weights)
    s_2 = EpochSampler(P, B, SEED + 5, 0, 1, device=device, drop_last=False)
    second.attach_sampler(s_2)
    second.load_state_dict(state)
    assert s_2._host_cursor == 20 and int(s_2.cursor.item()) == 20 and torch.equal(s_2.perm, s_1.perm)
    second.step_from(ds, s_2, supports)
    assert s_2.clip_w.tolist() == [1, 1, 1, 0] and second.samples_seen == whole.samples_seen == P and second.step_count == whole.step_count == 6
    _same_state(second, whole, "resumed in front of the short step")
    assert set(EpochSampler(P, B, SEED, 0, 1, device=device).begin_epoch(0).state_dict()) == {"seed", "epoch", "cursor"}
    assert set(s_2.state_dict()) == {"seed", "epoch", "cursor"}


# ---- 9. captured -------------------------------------------------------------------------------------------------------------------------
def check_captured_epoch(device, adj3d):
    """GPU only: `capture_epoch` + `replay_step` with a drop_last=False sampler over two epochs (6 steps each, `begin_epoch` between
    them) equals the eager `step_from` run -- every loss `torch.equal`, the short steps included, state equal at the end -- with the
    optimiser tail outside the graph and inside it; the addresses of pools, batch tensors, perm, cursor, clip_w, denom and n_valid do
    not change; samples_seen == 46."""
    make, ds, supports = _step_case("detection", adj3d, device)
    (_, eager) = make()
    s_e = _tail_sampler(device)
    want = []
    for e in range(2):
        eager.begin_epoch(e, 2, sampler=s_e)
        want += [eager.step_from(ds, s_e, supports).clone() for _ in range(s_e.steps_per_epoch)]
    assert len(want) == 12 and eager.samples_seen == 2 * P
    for include_update in (False, True):
        (_, st) = make()
        s_c = _tail_sampler(device, 8)
        keep = st.snapshot()
        st.capture_epoch(ds, s_c, supports, include_update=include_update)
        assert int(s_c.cursor.item()) == 8 and s_c._host_cursor == 8      # the warm-up gathers moved it; it is back
        st.restore(keep)
        inputs = st._graphs[0][2]
        addrs = lambda: [t.data_ptr() for t in (ds.x, ds.y, inputs[0], inputs[1], inputs[2], s_c.perm, s_c.cursor, s_c.clip_w,     # noqa: E731
                                                 s_c.denom, s_c.n_valid)]
        addr0 = addrs()
        got = []
        for e in range(2):
            st.begin_epoch(e, 2)
            for k in range(s_c.steps_per_epoch):
                got.append(st.replay_step().clone())
                assert int(s_c.cursor.item()) == (k + 1) * B
            assert s_c.clip_w.tolist() == [1, 1, 1, 0] and int(s_c.n_valid.item()) == 3 and float(s_c.denom.item()) == 3.0
        assert addrs() == addr0
        for k, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(u, v), (include_update, k, u.item(), v.item())
        assert st.step_count == eager.step_count == 12 and st.samples_seen == eager.samples_seen == 46
        _same_state(st, eager, f"captured epoch with its short step (include_update={include_update})")


# ---- 10. refusals and operator registration ----------------------------------------------------------------------------------------------
def check_refusals(device):
    """each refusal names the argument: weights of another dtype, shape or device, a divisor that is not one float32, one of the
    pair missing, validity outputs of the wrong dtype or size, an increment that is not one int64; the C entry points refuse null
    pointers and a tensor that is not B clips of equal size.  Past the end of the epoch (every weight 0) nothing raises."""
    from eeg_gnn_ssl_amd import _lib, ops
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    head = lambda **kw: ops.cls_head_loss(z(HEAD_B, N, HEAD_H), z(1, HEAD_H), z(1), z(HEAD_B), "detection", **kw)     # noqa: E731
    with pytest.raises(RuntimeError, match=r"cls_head_loss: clip_w must be a float32 tensor of shape \(6,\)"):
        head(clip_w=z(HEAD_B, dtype=torch.float64), denom=z(1))
    with pytest.raises(RuntimeError, match=r"cls_head_loss: clip_w must be a float32 tensor of shape \(6,\)"):
        head(clip_w=z(HEAD_B - 1), denom=z(1))
    with pytest.raises(RuntimeError, match=r"cls_head_loss: clip_w must be .* got torch.float32 \(6,\) on meta"):
        head(clip_w=torch.zeros(HEAD_B, device="meta"), denom=z(1))
    with pytest.raises(RuntimeError, match=r"cls_head_loss: denom must be one float32"):
        head(clip_w=z(HEAD_B), denom=z(2))
    with pytest.raises(RuntimeError, match=r"cls_head_loss: clip_w and denom come together"):
        head(clip_w=z(HEAD_B))
    with pytest.raises(RuntimeError, match=r"bce_logits: clip_w must be a float32 tensor of shape \(4,\)"):
        ops.bce_with_logits(z(4), z(4), clip_w=z(3), denom=z(1))
    with pytest.raises(RuntimeError, match=r"cross_entropy: denom must be one float32"):
        ops.cross_entropy(z(4, 3), z(4, dtype=torch.int64), clip_w=z(4), denom=z(1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"masked_loss: clip_w must be a float32 tensor of shape \(5,\)"):
        ops.masked_regression_loss(z(*REG_SHAPE), z(*REG_SHAPE), clip_w=z(4), denom=z(1))
    with pytest.raises(RuntimeError, match=r"masked_regression_loss: clip_w and denom come together"):
        ops.masked_regression_loss(z(*REG_SHAPE), z(*REG_SHAPE), denom=z(1))
    with pytest.raises(RuntimeError, match=r"teacher_flags: increment must be an int or one int64"):
        ops.teacher_flags(z(2, dtype=torch.int64), z(1, dtype=torch.int64), z(1, dtype=torch.int32), 30.0, 4)
    perm, cursor = torch.arange(P, device=device), z(1, dtype=torch.int64)
    tail = lambda **kw: ops.gather_clips(z(P, 4), z(B, 4), perm, cursor, **{**dict(clip_w=z(B), denom=z(1), n_valid=z(1, dtype=torch.int64)), **kw})     # noqa: E731
    with pytest.raises(RuntimeError, match=r"gather_clips: n_valid must be a contiguous torch.int64 tensor of shape \(1,\)"):
        tail(n_valid=z(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"gather_clips: clip_w must be a contiguous torch.float32 tensor of shape \(4,\)"):
        tail(clip_w=z(B + 1))
    with pytest.raises(RuntimeError, match=r"gather_clips: denom must be"):
        tail(denom=z(2))
    with pytest.raises(RuntimeError, match=r"gather_clips: clip_w, denom and n_valid come together"):
        tail(denom=None)
    assert int(cursor.item()) == 0                                  # no refused call moved it
    # C ABI
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    xp, xo, cw, dn, nv, f1 = z(P, 4), z(B, 4), z(B), z(1), z(1, dtype=torch.int64), z(1)
    gather = lambda *a: lib.query("eeg_dcrnn_gather_clips_tail", p(xp), p(xo), 16, None, None, 0, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 1, *a, None)     # noqa: E731
    refused(gather(None, p(dn), p(nv)), "null clip_w / denom / n_valid")
    refused(gather(p(cw), p(dn), None), "null clip_w / denom / n_valid")
    reg = z(*REG_SHAPE)
    ws = z(lib.query("eeg_dcrnn_masked_loss_ws_floats"))
    n = reg.numel()
    refused(lib.query("eeg_dcrnn_masked_loss_w", p(reg), p(reg), n, 7, p(cw), p(dn), 0, 0.0, 1.0, 0.0, 0, p(f1), p(reg), p(ws), None), "not B=7 clips")
    refused(lib.query("eeg_dcrnn_masked_loss_w", p(reg), p(reg), n, 5, None, p(dn), 0, 0.0, 1.0, 0.0, 0, p(f1), p(reg), p(ws), None), "null clip_w / denom")
    refused(lib.query("eeg_dcrnn_bce_logits_w", p(cw), p(cw), B, p(cw), None, p(f1), p(cw), None), "null clip_w / denom")
    refused(lib.query("eeg_dcrnn_ce_logits_w", p(cw), p(nv), 1, 4, None, p(dn), p(f1), p(cw), None), "null clip_w / denom")
    refused(lib.query("eeg_dcrnn_teacher_flags_dev", p(nv), p(nv), None, 30.0, 4, p(cw), None), "null increment")
    assert int(cursor.item()) == 0


def check_past_the_end(device, adj3d, units=64):
    """a step issued past the end of the epoch (cursor 24 >= P: the caller's error) stays finite: every weight 0, loss 0, a zero
    gradient bucket, no exception; it counts no samples"""
    make, ds, supports = _step_case("classification", adj3d, device, units)
    (_, st) = make()
    s = _tail_sampler(device, 24)
    loss = st.step_from(ds, s, supports)
    assert float(loss) == 0.0 and float(st.fp.flat_grad.abs().max()) == 0.0 and s.clip_w.tolist() == [0, 0, 0, 0]
    assert st.samples_seen == 0 and st.step_count == 1 and bool(torch.isfinite(st.fp.flat).all())


def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on the new operators"""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    d = lambda t: t.to(device)     # noqa: E731
    perm = d(torch.randperm(P, generator=g))
    i64 = lambda *v: d(torch.tensor(list(v), dtype=torch.int64))     # noqa: E731
    cw, dn = _f(HEAD_W, device), _f([4.0], device)
    z, w, bias, y = _head_case(4, device, g)
    pred, yt = _reg_case(device, g)
    samples = [
        (E.gather_clips_tail.default, (d(torch.randn(P, T, 4, D, generator=g)), d(torch.zeros(B, T, 4, D)), None, None, d(torch.rand(P, generator=g)),
                                       d(torch.zeros(B)), d(torch.randint(1, 4, (P,), generator=g)), i64(0, 0, 0, 0), perm, i64(20), 0, 1,
                                       d(torch.zeros(B)), d(torch.zeros(1)), i64(0))),
        (E.gather_clips_tail.default, (d(torch.randn(P, 4, T * W, generator=g)), d(torch.zeros(B, 4, T * W)), d(torch.randn(P, 4, TY * W, generator=g)),
                                       d(torch.zeros(B, 4, TY * W)), None, None, None, None, perm, i64(16), 1, 2,
                                       d(torch.zeros(B)), d(torch.zeros(1)), i64(0))),
        (E.cls_head_loss_w.default, (z, w, bias, y, 1, 0.0, None, cw, dn, torch.empty_like(w), torch.empty_like(bias))),
        (E.bce_logits_w.default, (d(torch.randn(HEAD_B, generator=g)), d(torch.rand(HEAD_B, generator=g)), cw, dn)),
        (E.ce_logits_w.default, (d(torch.randn(HEAD_B, 4, generator=g)), y, cw, dn)),
        (E.masked_loss_w.default, (pred, yt, True, 0.3, 1.7, 0.0, 1, _f(REG_W, device), _f([3.0], device))),
        (E.teacher_flags_dev_.default, (i64(977, 5), i64(40), i64(3), 30.0, 6)),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
