"""Checks of class imbalance on the device: the multiplicative criteria (`torch.ops.eeg_dcrnn.bce_logits_cw`, `ce_logits_cw`,
`cls_head_loss_cw`; `ops.bce_with_logits` / `cross_entropy` / `cls_head_loss` with `clip_u=, denom=`), the launch that writes a step's
weights (`ops.clip_weights`), `TrainStep(class_weights=, weight_norm=, sample_weights=)` and `BalancedEpochSampler`.  As in
last_batch_suite.py the same functions run on the GPU library and on the emulator build of the same kernel sources
(tests/test_class_weights.py).

Tolerances: `torch.equal` wherever the arithmetic is the same (all-ones weights; a slot of weight 0; `clip_weights` on dyadic weights,
whose sums are exact in any order; the sampler's permutation, which is integer arithmetic); `parity_suite.TOL` (2e-5 of the tensor's
largest magnitude, `assert_close_scaled`) against the framework's weighted criteria evaluated in float64.

Shapes: the head at N = 19, H = 64, C in {1, 4} and B in {1, 5, 9} (a workgroup of four clips with three, and with one, wave short
besides full ones), the stand-alone criteria also at B = 257 (one above their block of 256 threads), the weights kernel at B = 4,
world in {1, 2, 3} over an epoch of 10 clips out of a pool of 13.

Each check FAILS ON THE PARENT COMMIT: the operators, the `clip_u` argument, the TrainStep arguments and the sampler do not exist there."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from device_epoch_suite import B, P, SEED, T, _same_state, _state, _step_case
from parity_suite import TOL, assert_close_scaled, kernels_run

N, H = 19, 64
HEAD_BATCHES = (1, 5, 9)
CRIT_BATCHES = (1, 5, 9, 257)
CLASS_W = [0.25, 2.0, 0.5, 4.0]         # dyadic: products and sums of a handful of them are exact in float32
POS_W = 4.0


def _f(values, device):
    return torch.tensor(values, dtype=torch.float32, device=device)


def _cpu(t):
    return t.detach().cpu().numpy()


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _head_case(b, c, device, g):
    z = torch.randn(b, N, H, generator=g).to(device)
    w, bias = (0.3 * torch.randn(c, H, generator=g)).to(device), (0.1 * torch.randn(c, generator=g)).to(device)
    if c == 1:
        y = (torch.arange(b) % 2 == 0).float()                     # both classes whenever b > 1
    else:
        y = torch.arange(b) % c
    return z, w, bias, y.to(device)


def _weights_of(y, c, device):
    """(clip_u, denom) the way the framework weighs: C = 4: u = w[y], denom = sum u (`weight=`); C = 1: u = y ? p : 1, denom = B"""
    if c == 1:
        return torch.where(y > 0.5, _f(POS_W, device), _f(1.0, device)), _f([float(y.numel())], device)
    u = _f(CLASS_W, device)[y]
    return u, u.sum().reshape(1)


def _head(z, w, bias, y, p_drop=0.0, clip_u=None, denom=None, select=False):
    """the fused head operator -> dict of everything it writes + the {seed, offset} pair of its masks (a fresh generator state per
    call: the same dropout masks on every call, last_batch_suite._head's way)"""
    from eeg_gnn_ssl_amd import ops
    E = torch.ops.eeg_dcrnn
    state = torch.tensor([4242, 11], dtype=torch.int64, device=z.device)
    used = ops.rng_take(state, z.numel() // 4) if p_drop > 0 else None
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    kind = 0 if w.shape[0] == 1 else 1
    if clip_u is None:
        loss, logits, arg, dlogits, dz = E.cls_head_loss(z, w, bias, y, kind, p_drop, used, dw, db)
    else:
        op = E.cls_head_loss_w if select else E.cls_head_loss_cw
        loss, logits, arg, dlogits, dz = op(z, w, bias, y, kind, p_drop, used, clip_u, denom, dw, db)
    return dict(loss=loss, logits=logits, arg=arg, dlogits=dlogits, dz=dz, dW=dw, dbias=db), used


def _framework_criterion(logits64, y, c):
    """the framework's weighted criterion on float64 logits (B, C)"""
    if c == 1:
        return F.binary_cross_entropy_with_logits(logits64.view(-1), y.double(), pos_weight=torch.tensor(POS_W, dtype=torch.float64, device=y.device))
    return F.cross_entropy(logits64, y, weight=torch.tensor(CLASS_W, dtype=torch.float64, device=y.device))


def _framework_head(z, w, bias, y, mask):
    """model.py:267-270 + the weighted criterion through autograd in float64; mask: the kernels' keep / (1 - p) factors (or None)"""
    c = w.shape[0]
    z64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (z, w, bias))
    zz = torch.relu(z64 if mask is None else z64 * mask.double().view_as(z64))
    logits = (zz @ w64.t() + b64).max(dim=1).values
    loss = _framework_criterion(logits, y, c)
    dlogits, = torch.autograd.grad(loss, logits, retain_graph=True)
    loss.backward()
    return dict(loss=loss.detach().reshape(1), logits=logits.detach(), dlogits=dlogits, dz=z64.grad, dW=w64.grad, dbias=b64.grad)


# ---- 1. against the framework ----------------------------------------------------------------------------------------------------------
def check_framework(device):
    """`ce_logits_cw` and the fused head with u = w[y], denom = sum u against `F.cross_entropy(weight=w)`; `bce_logits_cw` and the fused
    head with u = (1, p)[y], denom = B against `F.binary_cross_entropy_with_logits(pos_weight=p)` on 0 / 1 labels -- both in float64,
    at TOL of the largest magnitude: loss, dlogits, dz, dW, dbias; the head with dropout off and at 0.5 (the reference multiplies
    with the factors `ops.dropout_mask` materialises for the call's own {seed, offset} pair)."""
    from eeg_gnn_ssl_amd import ops
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(51)
    for c in (1, 4):
        for b in HEAD_BATCHES:
            z, w, bias, y = _head_case(b, c, device, g)
            clip_u, denom = _weights_of(y, c, device)
            for p_drop in (0.0, 0.5):
                got, used = _head(z, w, bias, y, p_drop, clip_u, denom)
                mask = ops.dropout_mask(used, z.numel(), p_drop) if p_drop > 0 else None
                want = _framework_head(z, w, bias, y, mask)
                for k, ref in want.items():
                    assert_close_scaled(_cpu(got[k]), _cpu(ref.reshape(got[k].shape)), f"head C={c} B={b} p={p_drop} {k}")
                assert float(got["dz"].abs().max()) > 0 and np.isfinite(float(got["loss"]))
        for b in CRIT_BATCHES:
            y = ((torch.arange(b) % 2 == 0).float() if c == 1 else torch.arange(b) % c).to(device)
            lg = (2.0 * torch.randn(b, c, generator=g)).to(device)
            clip_u, denom = _weights_of(y, c, device)
            l64 = lg.double().requires_grad_(True)
            want = _framework_criterion(l64, y, c)
            want.backward()
            loss, dx = E.bce_logits_cw(lg.view(-1), y, clip_u, denom) if c == 1 else E.ce_logits_cw(lg, y, clip_u, denom)
            assert_close_scaled(_cpu(loss.reshape(1)), _cpu(want.reshape(1)), f"criterion C={c} B={b} loss")
            assert_close_scaled(_cpu(dx.view(b, c)), _cpu(l64.grad), f"criterion C={c} B={b} dlogits")
            fn = ops.bce_with_logits if c == 1 else ops.cross_entropy
            assert torch.equal(fn(lg.view(-1) if c == 1 else lg, y, clip_u=clip_u, denom=denom), loss)
    # autograd through the public criterion: d loss / d logits is the kernel's own
    lg = torch.randn(5, 4, generator=g).to(device).requires_grad_(True)
    y = (torch.arange(5) % 4).to(device)
    clip_u, denom = _weights_of(y, 4, device)
    ops.cross_entropy(lg, y, clip_u=clip_u, denom=denom).backward()
    assert torch.equal(lg.grad, E.ce_logits_cw(lg.detach(), y, clip_u, denom)[1])


# ---- 2. ones are free ------------------------------------------------------------------------------------------------------------------
def check_ones_are_free(device):
    """u = 1 and denom = B: every multiplicative operator equals its unweighted twin bit for bit (`torch.equal`) on everything it
    writes -- the fused head (C = 1 and 4, B = 1, 5, 9, dropout 0 and 0.5 with the same generator state) and both criteria (B up to
    257)."""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(52)
    for c in (1, 4):
        for b in HEAD_BATCHES:
            z, w, bias, y = _head_case(b, c, device, g)
            ones, denom = _f([1.] * b, device), _f([float(b)], device)
            for p_drop in (0.0, 0.5):
                want, got = _head(z, w, bias, y, p_drop)[0], _head(z, w, bias, y, p_drop, ones, denom)[0]
                for k in want:
                    assert torch.equal(got[k], want[k]), (c, b, p_drop, k)
                assert np.isfinite(float(want["loss"])) and float(want["dz"].abs().max()) > 0
        for b in CRIT_BATCHES:
            y = ((torch.arange(b) % 2 == 0).float() if c == 1 else torch.arange(b) % c).to(device)
            lg = (2.0 * torch.randn(b, c, generator=g)).to(device)
            ones, denom = _f([1.] * b, device), _f([float(b)], device)
            plain, weighted = (E.bce_logits(lg.view(-1), y), E.bce_logits_cw(lg.view(-1), y, ones, denom)) if c == 1 else \
                              (E.ce_logits(lg, y), E.ce_logits_cw(lg, y, ones, denom))
            assert torch.equal(weighted[0], plain[0]) and torch.equal(weighted[1], plain[1]), (c, b)


# ---- 3. zero selects out ---------------------------------------------------------------------------------------------------------------
def check_zero_selects_out(device):
    """a slot with u = 0 holding label 99 (cross-entropy), a NaN label (BCE) or -- the stand-alone criteria, whose logits are an input
    -- NaN logits: loss, dlogits, dz, dW, dbias are finite and `torch.equal` to the same call with a harmless label in that slot;
    its dlogits and dz are exactly zero; the head's logits and arg are written for it as for every clip.  The other slots carry the
    weights of check_framework.  On a clip that COUNTS the label 99 keeps today's rule: NaN loss."""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(53)
    for c in (1, 4):
        for b, slot in ((5, 1), (9, 8)):
            z, w, bias, y = _head_case(b, c, device, g)
            clip_u, denom = _weights_of(y, c, device)
            clip_u = clip_u.clone()
            clip_u[slot] = 0.0
            bad = y.clone()
            bad[slot] = float("nan") if c == 1 else 99
            want, got = _head(z, w, bias, y, 0.0, clip_u, denom)[0], _head(z, w, bias, bad, 0.0, clip_u, denom)[0]
            for k in want:
                assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k].float()).all()), (c, b, k)
            assert float(got["dlogits"][slot].abs().max()) == 0.0 and float(got["dz"][slot].abs().max()) == 0.0
            assert float(got["dz"].abs().max()) > 0
            plain = _head(z, w, bias, y)[0]
            assert torch.equal(got["logits"], plain["logits"]) and torch.equal(got["arg"], plain["arg"])
            # the stand-alone criterion: NaN logits in that slot as well
            lg = plain["logits"].clone()
            nan_lg = lg.clone()
            nan_lg[slot] = float("nan")
            crit = (lambda l_, y_: E.bce_logits_cw(l_.view(-1), y_, clip_u, denom)) if c == 1 else (lambda l_, y_: E.ce_logits_cw(l_, y_, clip_u, denom))     # noqa: E731
            (lw, dw_), (lb, db_) = crit(lg, y), crit(nan_lg, bad)
            assert torch.equal(lw, lb) and torch.equal(dw_, db_) and bool(torch.isfinite(lb).all()) and bool(torch.isfinite(db_).all())
            assert float(db_.view(b, c)[slot].abs().max()) == 0.0
            if c == 4:
                bad[(slot + 1) % b] = 99                             # a clip that counts: NaN, as the unweighted kernels
                assert bool(torch.isnan(_head(z, w, bias, bad, 0.0, clip_u, denom)[0]["loss"])) and bool(torch.isnan(crit(lg, bad)[0]))
        # every weight zero: loss 0, every gradient 0
        z, w, bias, y = _head_case(5, c, device, g)
        none = _head(z, w, bias, y, 0.0, _f([0.] * 5, device), _f([1.], device))[0]
        assert all(float(none[k].abs().max()) == 0.0 for k in ("loss", "dlogits", "dz", "dW", "dbias")), c


# ---- 4. the step's weights ---------------------------------------------------------------------------------------------------------------
W_B, W_P, W_LEN = 4, 13, 10


def _np_weights(labels, perm, c0, slots, world, class_w, sample_w, norm):
    """numpy restatement of `clip_weights` over all `slots` of a step: (u (slots,) float32, denom float32)"""
    u = np.zeros(slots, dtype=np.float32)
    n_valid = 0
    for s in range(slots):
        pos = c0 + s
        if perm is not None and not 0 <= pos < len(perm):
            continue
        src = s if perm is None else min(max(int(perm[pos]), 0), len(labels) - 1)
        cls = int(labels[src]) if labels.dtype == np.int64 else (1 if labels[src] >= 0.5 else 0)
        cw = np.float32(class_w[cls]) if class_w is not None and 0 <= cls < len(class_w) else np.float32(1.0)
        u[s] = cw * (np.float32(sample_w[src]) if sample_w is not None else np.float32(1.0))
        n_valid += 1
    d = float(max(n_valid, 1)) if norm == "count" else (float(u.astype(np.float64).sum()) or 1.0)
    return u, np.float32(d / world)


def check_clip_weights(device):
    """`ops.clip_weights` against the numpy restatement, exact, with dyadic class weights (0.25, 2, 0.5, 4) and sample weights out of
    (0.25, 0.5, 2, 4, 0): int64 labels (one of them 7: no class, weight 1) and float 0 / 1 labels; both normalisations; class weights
    alone, sample weights alone, both; an epoch of 10 clips out of a pool of 13 at B = 4, world 1, 2, 3 with the cursor at 0, at 8
    (the short last step; world 3 is short from the start: 12 slots for 10 clips) and at 12 (past the end: every weight 0, divisor
    1 / world); back = 0 with the cursor as the gather saw it and back = B * world with the advanced one give the same bits; the
    ranks' slices tile the single-process vector (B * world slots, world 1) and denom * world is equal on every rank.  The batch
    form: the batch's own labels, divisor local.  Outputs sit between sentinels."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(54)
    perm = torch.randperm(W_P, generator=g)[:W_LEN]
    lab_i = torch.randint(0, 4, (W_P,), generator=g)
    lab_i[int(perm[9])] = 7
    lab_f = (torch.rand(W_P, generator=g) < 0.4).float()
    sample = torch.tensor([0.25, 0.5, 2.0, 4.0, 0.0])[torch.randint(0, 5, (W_P,), generator=g)]
    sample[int(perm[0])] = 0.0
    d = lambda t: None if t is None else t.to(device)     # noqa: E731
    cases = 0
    for labels, class_w in ((lab_i, torch.tensor(CLASS_W)), (lab_f, torch.tensor([0.5, POS_W]))):
        for cw, sw in ((class_w, None), (None, sample), (class_w, sample)):
            for norm in ("sum", "count"):
                for c0 in (0, 8, 12):
                    for world in (1, 2, 3):
                        slots = W_B * world
                        want_u, want_d = _np_weights(labels.numpy(), perm.numpy(), c0, slots, world, None if cw is None else cw.numpy(),
                                                     None if sw is None else sw.numpy(), norm)
                        whole = torch.full((slots + 2,), -77.0, device=device)
                        ops.clip_weights(d(labels), whole[1:-1], torch.zeros(1, device=device), d(cw), d(sw), norm, perm=d(perm),
                                         cursor=torch.tensor([c0], device=device), rank=0, world=1)
                        assert np.array_equal(_cpu(whole[1:-1]), want_u) and whole[0] == -77 and whole[-1] == -77, (norm, c0, world)
                        denoms = []
                        for rank in range(world):
                            for back in (0, slots):
                                buf, dn = torch.full((W_B + 2,), -77.0, device=device), torch.full((3,), -77.0, device=device)
                                cursor = torch.tensor([c0 + back], device=device)
                                ops.clip_weights(d(labels), buf[1:-1], dn[1:2], d(cw), d(sw), norm, perm=d(perm), cursor=cursor, back=back,
                                                 rank=rank, world=world)
                                tag = (str(labels.dtype), cw is not None, sw is not None, norm, c0, world, rank, back)
                                assert np.array_equal(_cpu(buf[1:-1]), want_u[rank * W_B:(rank + 1) * W_B]), (tag, buf, want_u)
                                assert _cpu(dn)[1] == want_d and np.isfinite(want_d) and want_d > 0, (tag, dn, want_d)
                                assert buf[0] == -77 and buf[-1] == -77 and dn[0] == -77 and dn[2] == -77 and int(cursor) == c0 + back, tag
                                denoms.append(float(dn[1]) * world)
                                cases += 1
                        assert len(set(denoms)) == 1
                        if c0 == 12:
                            assert not want_u.any() and want_d == np.float32(1.0 / world)
            # the batch form
            for norm in ("sum", "count"):
                if sw is not None:
                    continue
                batch = labels[:5]
                want_u, want_d = _np_weights(batch.numpy(), None, 0, 5, 1, cw.numpy(), None, norm)
                u, dn = torch.empty(5, device=device), torch.empty(1, device=device)
                ops.clip_weights(d(batch), u, dn, d(cw), norm=norm, world=3)            # (world: ignored, the divisor is the rank's own)
                assert np.array_equal(_cpu(u), want_u) and _cpu(dn)[0] == want_d
    assert cases > 200
    # a sum of zero gives the divisor 1: class weights that miss every label present
    u, dn = torch.empty(3, device=device), torch.empty(1, device=device)
    ops.clip_weights(torch.zeros(3, dtype=torch.int64, device=device), u, dn, _f([0.0, 1.0], device))
    assert u.tolist() == [0, 0, 0] and float(dn) == 1.0


# ---- 5. the step -----------------------------------------------------------------------------------------------------------------------
def _class_weights(mode):
    return [1.0, POS_W] if mode == "detection" else CLASS_W


def _framework_step(st, model, x, y, lens, supports, mode):
    """loss and flat gradient of autograd through `model(x)` and the framework's weighted criterion in float64 (the model's
    parameters' .grad are views of the step's flat bucket)"""
    st.fp.zero_grad()
    with torch.no_grad():
        feats, _, sup = st._data_chain(x, y, lens, supports)
    out = model(feats, lens, sup)
    loss = _framework_criterion(out.double(), y, 1 if mode == "detection" else 4)
    with st.fp.sink:
        loss.backward()
    return loss.detach().reshape(1), st.fp.flat_grad.clone()


def check_step(device, adj3d, units=64):
    """`TrainStep(class_weights=w).forward_backward` (eager) against autograd through `model(x)` with `F.cross_entropy(weight=w)` /
    `F.binary_cross_entropy_with_logits(pos_weight=p)` in float64: loss and `flat_grad` at TOL -- detection (features, the 2-D
    distance graph) and classification (raw signals, variable lengths, supports=None), with the fused head and without it.
    All-ones weights with count normalisation: loss, logits and `flat_grad` `torch.equal` to the step without weights."""
    from eeg_gnn_ssl_amd.train_step import TrainStep
    for mode in ("detection", "classification"):
        make, ds, supports = _step_case(mode, adj3d, device, units)
        idx = torch.arange(5, 5 + B, device=device)
        x, y = ds.x[idx], ds.y[idx]
        lens = torch.full((B,), T, dtype=torch.int64, device=device) if ds.seq_lengths is None else ds.seq_lengths[idx]
        assert y.unique().numel() > 1
        (model, plain) = make()
        kw = dict(raw_window=plain.raw_window, raw_mean=plain.raw_mean, raw_std=plain.raw_std, padding_val=plain.padding_val)
        want_l, want_g = _framework_step(plain, model, x, y, lens, supports, mode)
        for fused in (True, False):
            (m2, _) = make()
            st = TrainStep(m2, task=mode, class_weights=_class_weights(mode), **kw)
            assert st.weight_norm == ("count" if mode == "detection" else "sum")
            st.fused_head = fused
            loss = st.forward_backward(x, y, lens, supports)
            assert_close_scaled(_cpu(loss.reshape(1)), _cpu(want_l), f"step {mode} fused={fused}: loss")
            assert_close_scaled(_cpu(st.fp.flat_grad), _cpu(want_g), f"step {mode} fused={fused}: flat_grad")
            assert float(want_g.abs().max()) > 0 and st.samples_seen == 0
            # all-ones weights, count normalisation: the unweighted step, bit for bit
            (m3, ref), (m4, _) = make(), make()
            ones = TrainStep(m4, task=mode, class_weights=[1.0] * len(_class_weights(mode)), weight_norm="count", **kw)
            ref.fused_head = ones.fused_head = fused
            l_ref, l_one = ref.step(x, y, lens, supports), ones.step(x, y, lens, supports)
            assert torch.equal(l_one, l_ref) and torch.equal(ones.fp.flat_grad, ref.fp.flat_grad), (mode, fused)
            assert ones.samples_seen == ref.samples_seen == B
            if fused:
                assert torch.equal(ones.last_logits, ref.last_logits)
            _same_state(ones, ref, f"all-ones weights {mode} fused={fused}")


def _weighted_pair(mode, adj3d, device, units, norm=None, sample=False):
    """-> (make(): a fresh weighted TrainStep, dataset, supports, sample weight pool or None)"""
    from eeg_gnn_ssl_amd.train_step import TrainStep
    make, ds, supports = _step_case(mode, adj3d, device, units)
    sw = None
    if sample:
        sw = torch.tensor([0.5, 1.0, 2.0, 0.0])[torch.arange(P) % 4].to(device)

    def weighted():
        (model, plain) = make()
        kw = dict(raw_window=plain.raw_window, raw_mean=plain.raw_mean, raw_std=plain.raw_std, padding_val=plain.padding_val)
        return TrainStep(model, task=mode, class_weights=_class_weights(mode), weight_norm=norm, sample_weights=sw, **kw)
    return weighted, ds, supports, sw


def check_sampler_step(device, adj3d, units=64):
    """`step_from` with class AND sample weights through a drop_last=False sampler against a hand-fed `step` on the same clips with the
    expected weights handed over as the batch's own: the short last step (3 clips of B = 4, the fourth slot's weight 0) gives the
    loss of the 3-clip batch at TOL and counts 3 samples; a full step is `torch.equal` to `forward_backward` in the batch form when
    there are no sample weights (the same weights, the same divisor bits)."""
    from eeg_gnn_ssl_amd import EpochSampler
    weighted, ds, supports, sw = _weighted_pair("classification", adj3d, device, units, sample=True)
    st = weighted()
    s = EpochSampler(P, B, SEED, 0, 1, device=device, drop_last=False).begin_epoch(0).seek(20)
    loss = st.step_from(ds, s, supports)
    clip_u, denom = st._weight_buffers[B]
    idx = s.perm[20:23]
    want_u = _f(CLASS_W, device)[ds.y[idx]] * sw[idx]
    assert torch.equal(clip_u[:3], want_u) and float(clip_u[3]) == 0.0 and float(denom) == float(want_u.sum()) > 0
    assert st.samples_seen == 3 and int(s.cursor.item()) == 24
    # the same three clips by hand: per-clip terms through the stand-alone criterion on the step's own logits
    lg = st.last_logits[:3]
    want = torch.ops.eeg_dcrnn.ce_logits_cw(lg, ds.y[idx], want_u, want_u.sum().reshape(1))[0]
    assert_close_scaled(_cpu(loss.reshape(1)), _cpu(want.reshape(1)), "short weighted step: loss")
    # class weights alone, a full step: sampler form == batch form, bit for bit
    weighted, ds, supports, _ = _weighted_pair("detection", adj3d, device, units)
    a, b = weighted(), weighted()
    s = EpochSampler(P, B, SEED, 0, 1, device=device).begin_epoch(0)
    idx = s.perm[:B].clone()
    la = a.step_from(ds, s, supports)
    lb = b.step(ds.x[idx], ds.y[idx], torch.full((B,), T, dtype=torch.int64, device=device), supports)
    assert torch.equal(la, lb) and a.samples_seen == b.samples_seen == B
    _same_state(a, b, "sampler form against batch form")


# ---- 6. epochs ---------------------------------------------------------------------------------------------------------------------------
def check_captured_epoch(device, adj3d):
    """GPU only: `capture_epoch` + `replay_step` with class weights and a drop_last=False sampler over two epochs (6 steps each, the
    last on 3 clips) equals the eager `step_from` run loss by loss (`torch.equal`) and in its final state, with the optimiser tail
    outside the graph and inside it; samples_seen counts clips (46), the weight buffers keep their addresses."""
    from eeg_gnn_ssl_amd import EpochSampler
    weighted, ds, supports, _ = _weighted_pair("detection", adj3d, device, 64)
    tail = lambda: EpochSampler(P, B, SEED, 0, 1, device=device, drop_last=False).begin_epoch(0)     # noqa: E731
    eager, s_e = weighted(), tail()
    want = []
    for e in range(2):
        eager.begin_epoch(e, 2, sampler=s_e)
        want += [eager.step_from(ds, s_e, supports).clone() for _ in range(s_e.steps_per_epoch)]
    assert len(want) == 12 and eager.samples_seen == 2 * P and len(set(float(v) for v in want)) == 12
    for include_update in (False, True):
        st, s_c = weighted(), tail().seek(8)
        keep = st.snapshot()
        st.capture_epoch(ds, s_c, supports, include_update=include_update)
        assert int(s_c.cursor.item()) == 8 and s_c._host_cursor == 8
        st.restore(keep)
        addr0 = [t.data_ptr() for t in st._weight_buffers[B]]
        got = []
        for e in range(2):
            st.begin_epoch(e, 2)
            got += [st.replay_step().clone() for _ in range(s_c.steps_per_epoch)]
            assert float(st._weight_buffers[B][0][3]) == 0.0          # the short step's fourth slot
        assert [t.data_ptr() for t in st._weight_buffers[B]] == addr0
        for k, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(u, v), (include_update, k, u.item(), v.item())
        assert st.step_count == eager.step_count == 12 and st.samples_seen == eager.samples_seen == 46
        _same_state(st, eager, f"captured weighted epoch (include_update={include_update})")


def two_rank_step(device, adj3d, rank, world, norm, units=16):
    """one rank's `forward_backward` on the short last step of a drop_last=False epoch (cursor 16 of P = 23: 4 + 3 clips on two ranks)
    with class weights -> (loss, flat gradient)"""
    from eeg_gnn_ssl_amd import EpochSampler
    weighted, ds, supports, _ = _weighted_pair("detection", adj3d, device, units, norm=norm)
    st = weighted()
    s = EpochSampler(P, B * (2 // world), SEED, rank, world, device=device, drop_last=False).begin_epoch(0).seek(16)
    batch = st._epoch_batch(ds, s)
    st._gather_batch(ds, s, batch)
    loss = st.forward_backward(batch[0], batch[1], batch[2], supports, sampler=s, label_pool=ds.y)
    return loss.clone(), st.fp.flat_grad.clone()


def check_two_ranks_against(device, adj3d, by_rank, norm, units=16):
    """the mean of two ranks' losses and gradients (the summed all-reduce and its 1 / world) against one process at 2 * B, at TOL"""
    want_l, want_g = two_rank_step(device, adj3d, 0, 1, norm, units)
    assert_close_scaled(_cpu((by_rank[0][0] + by_rank[1][0]) / 2).reshape(1), _cpu(want_l).reshape(1), f"two ranks, {norm}: loss")
    assert_close_scaled(_cpu((by_rank[0][1] + by_rank[1][1]) / 2), _cpu(want_g), f"two ranks, {norm}: gradient")
    assert float(want_g.abs().max()) > 0 and float(by_rank[1][1].abs().max()) > 0


# ---- 7. the balanced sampler -------------------------------------------------------------------------------------------------------------
BAL_SEED = 20240917                 # the committed seed of the sampler checks (the spread bound below was confirmed for it on the emulator)


def _np_balanced(labels, quotas, seed, epoch, redraw, device):
    """numpy restatement of `BalancedEpochSampler.begin_epoch` from `ops.epoch_keys` output"""
    from eeg_gnn_ssl_amd import ops
    n = labels.numel()
    keys = lambda e: ops.epoch_keys(torch.empty(n, dtype=torch.int64, device=device), seed, e).cpu().numpy()     # noqa: E731
    k1, k2 = keys(2 * epoch if redraw else 0), keys(2 * epoch + 1)
    cls = (labels.cpu().numpy() >= 0.5).astype(np.int64) if labels.dtype == torch.float32 else labels.cpu().numpy()
    chosen = []
    for c, q in enumerate(quotas):
        members = [i for i in range(n) if cls[i] == c]
        chosen += sorted(members, key=lambda i: (k1[i], i))[:q]
    return np.array(sorted(chosen, key=lambda i: (k2[i], i)), dtype=np.int64)


def check_balanced_sampler(device):
    """`BalancedEpochSampler` on 40 detection clips with 6 positives and on classification counts (3, 7, 12, 18): quotas min(n_c,
    int(scale_ratio * n_rarest)); perm equals the numpy restatement for epochs 0..3 with redraw on and off, holds exactly q_c clips of
    class c and no duplicates, and keeps its address; redraw=False keeps the selected set and changes the order, redraw=True changes
    the set; scale_ratio = 0.5 and explicit quotas; steps_per_epoch and take() follow epoch_len; a state_dict round trip in
    mid-epoch; the shards of world = 2 are disjoint and cover the step; n = 64 majority clips, q = 16, 200 epochs: every majority clip
    is chosen between 20 and 80 times (expectation 50, standard deviation 6.1: +-4.9 sd; the draw is deterministic for BAL_SEED)."""
    from eeg_gnn_ssl_amd import BalancedEpochSampler, DeviceDataset, ops
    g = torch.Generator().manual_seed(57)
    det = torch.zeros(40)
    det[torch.randperm(40, generator=g)[:6]] = 1.0
    cls = torch.cat([torch.full((n,), c) for c, n in enumerate((3, 7, 12, 18))])[torch.randperm(40, generator=g)]
    for labels, counts, want_q in ((det.to(device), [34, 6], [6, 6]), (cls.to(device), [3, 7, 12, 18], [3, 3, 3, 3])):
        for redraw in (True, False):
            s = BalancedEpochSampler(labels, 2, BAL_SEED, redraw=redraw, rank=0, world=1)
            assert s.class_counts == counts and s.quotas == want_q and s.epoch_len == sum(want_q) and s.P == 40
            assert s.steps_per_epoch == sum(want_q) // 2 and s.perm.numel() == s.epoch_len and s.epoch is None
            addr, sets, perms = s.perm.data_ptr(), [], []
            for e in range(4):
                s.cursor.fill_(5)
                perm = s.begin_epoch(e).perm.cpu().numpy()
                assert np.array_equal(perm, _np_balanced(labels, want_q, BAL_SEED, e, redraw, device)), (redraw, e)
                assert s.perm.data_ptr() == addr and int(s.cursor.item()) == 0 and s.epoch == e
                assert len(set(perm.tolist())) == len(perm)
                lab = labels.cpu()[torch.from_numpy(perm)]
                got = torch.bincount((lab >= 0.5).long() if lab.dtype == torch.float32 else lab, minlength=len(counts)).tolist()
                assert got == want_q, (redraw, e, got)
                sets.append(frozenset(perm.tolist()))
                perms.append(perm.tolist())
            assert len({tuple(p) for p in perms}) == 4
            assert (len(set(sets)) > 1) == redraw, (redraw, sets)
    # scale_ratio and explicit quotas
    half = BalancedEpochSampler(det.to(device), 2, BAL_SEED, scale_ratio=0.5, rank=0, world=1)
    assert half.quotas == [3, 3] and half.epoch_len == 6
    wide = BalancedEpochSampler(det.to(device), 2, BAL_SEED, scale_ratio=3.0, rank=0, world=1)
    assert wide.quotas == [18, 6]
    mine = BalancedEpochSampler(cls.to(device), 3, BAL_SEED, quotas=[3, 0, 5, 2], drop_last=False, rank=0, world=1).begin_epoch(1)
    lab = cls[mine.perm.cpu()]
    assert torch.bincount(lab, minlength=4).tolist() == [3, 0, 5, 2] and mine.epoch_len == 10 and mine.steps_per_epoch == 4
    assert [mine.take() for _ in range(5)] == [3, 3, 3, 1, 0] and mine.clip_w.numel() == 3
    assert np.array_equal(mine.perm.cpu().numpy(), _np_balanced(cls, [3, 0, 5, 2], BAL_SEED, 1, True, device))
    # state_dict in mid-epoch
    a = BalancedEpochSampler(cls.to(device), 3, BAL_SEED, quotas=[3, 0, 5, 2], rank=0, world=1).begin_epoch(2).seek(6)
    state = a.state_dict()
    assert state == {"seed": BAL_SEED, "epoch": 2, "cursor": 6}
    b = BalancedEpochSampler(cls.to(device), 3, BAL_SEED + 1, quotas=[3, 0, 5, 2], rank=0, world=1)
    b.load_state_dict(state)
    assert torch.equal(a.perm, b.perm) and int(b.cursor.item()) == 6 and b.epoch == 2 and b.seed == BAL_SEED
    # the shards of two ranks: disjoint, and together the step
    ds = DeviceDataset(torch.zeros(40, 1, 1, 4, device=device), torch.arange(40, dtype=torch.int64, device=device))
    r = [BalancedEpochSampler(cls.to(device), 2, BAL_SEED, quotas=[3, 3, 3, 3], rank=k, world=2).begin_epoch(3) for k in range(2)]
    assert torch.equal(r[0].perm, r[1].perm) and r[0].steps_per_epoch == 3
    x_out = torch.empty(2, 1, 1, 4, device=device)
    seen = []
    for step in range(3):
        ids = []
        for k in range(2):
            y_out = torch.empty(2, dtype=torch.int64, device=device)
            ds.gather(r[k], x_out, y_out)
            ids.append(y_out.cpu())
        assert torch.equal(torch.cat(ids), r[0].perm.cpu()[4 * step:4 * step + 4])
        seen += torch.cat(ids).tolist()
    assert len(set(seen)) == 12
    # the spread of the draw
    lab = torch.cat([torch.zeros(64), torch.ones(16)]).to(device)
    s = BalancedEpochSampler(lab, 4, BAL_SEED, rank=0, world=1)
    assert s.quotas == [16, 16]
    hits = torch.zeros(80, dtype=torch.int64)
    for e in range(200):
        hits[s.begin_epoch(e).perm.cpu()] += 1
    print("majority clips chosen over 200 epochs: min", int(hits[:64].min()), "max", int(hits[:64].max()))
    assert bool((hits[64:] == 200).all()) and int(hits[:64].sum()) == 200 * 16
    assert 20 <= int(hits[:64].min()) and int(hits[:64].max()) <= 80, hits[:64].tolist()


def check_balanced_captured(device, adj3d):
    """GPU only: a captured epoch step replays the NEXT epoch's perm after `begin_epoch` -- the labels gathered by the replays of epoch
    1 are the clips of its permutation, and the eager twin computes the same losses."""
    from eeg_gnn_ssl_amd import BalancedEpochSampler
    weighted, ds, supports, _ = _weighted_pair("detection", adj3d, device, 64)
    mk = lambda: BalancedEpochSampler(ds.y, B, BAL_SEED, rank=0, world=1).begin_epoch(0)     # noqa: E731
    eager, s_e, st, s_c = weighted(), mk(), weighted(), mk()
    assert s_c.epoch_len == 2 * min(s_c.class_counts) and s_c.steps_per_epoch >= 2
    keep = st.snapshot()
    st.capture_epoch(ds, s_c, supports)
    st.restore(keep)
    for e in range(2):
        eager.begin_epoch(e, 2, sampler=s_e)
        st.begin_epoch(e, 2)
        assert torch.equal(s_e.perm, s_c.perm)
        for k in range(s_c.steps_per_epoch):
            want, got = eager.step_from(ds, s_e, supports), st.replay_step()
            assert torch.equal(got, want), (e, k)
            assert torch.equal(st._graphs[0][2][1], ds.y[s_c.perm[k * B:(k + 1) * B]])
    _same_state(st, eager, "captured balanced epochs")


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d, units=64):
    """every refusal is a ValueError raised before any launch (the event recorder sees none): task ssl; a weight vector of the wrong
    length, dtype or device; negative, NaN, infinite weights; all-zero class weights; an unknown weight_norm; sample_weights with
    step() / capture(); sample_weights whose length is not the pool's; the sampler's own (a quota above the class count, an epoch
    shorter than a step); `clip_u` together with `clip_w` (host, RuntimeError like the operators' other refusals)."""
    from eeg_gnn_ssl_amd import BalancedEpochSampler, EpochSampler, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    make, ds, supports = _step_case("classification", adj3d, device, units)
    (model, plain) = make()
    kw = dict(raw_window=plain.raw_window, raw_mean=plain.raw_mean, raw_std=plain.raw_std, padding_val=plain.padding_val)
    ssl_model = _step_case("ssl", adj3d, device, units)[0]()[0]
    lens = torch.full((B,), T, dtype=torch.int64, device=device)
    good_sw = torch.ones(P, device=device)

    def refusals():
        def new(match, task="classification", m=model, **args):
            with pytest.raises(ValueError, match=match):
                TrainStep(m, task=task, **{**kw, **args})
        new(r"task='ssl'", task="ssl", m=ssl_model, class_weights=[1.0, 2.0], raw_window=None, padding_val=None)
        new(r"class_weights has shape \(3,\), expected \(4,\)", class_weights=[1.0, 2.0, 3.0])
        new(r"class_weights has shape \(4,\), expected \(2,\)", task="detection", class_weights=CLASS_W)
        new(r"class_weights must be float32", class_weights=torch.ones(4, dtype=torch.float64, device=device))
        new(r"class_weights must be float32 on .* got torch.float32 on meta", class_weights=torch.ones(4, device="meta"))
        new(r"class_weights must be finite and >= 0", class_weights=[1.0, -1.0, 1.0, 1.0])
        new(r"class_weights must be finite and >= 0", class_weights=[1.0, float("nan"), 1.0, 1.0])
        new(r"class_weights must be finite and >= 0", class_weights=[1.0, float("inf"), 1.0, 1.0])
        new(r"class_weights are all zero", class_weights=[0.0] * 4)
        new(r"weight_norm='mean'", class_weights=CLASS_W, weight_norm="mean")
        new(r"sample_weights must be a float32 \(P,\) tensor", sample_weights=[1.0] * P)
        new(r"sample_weights must be float32", sample_weights=torch.ones(P, dtype=torch.float64, device=device))
        new(r"sample_weights must be finite and >= 0", sample_weights=-good_sw)
        new(r"sample_weights has shape \(23, 1\)", sample_weights=good_sw.view(P, 1))
        st = TrainStep(model, task="classification", sample_weights=good_sw, **kw)
        with pytest.raises(ValueError, match=r"sample_weights=.*step\(\) / capture\(\)"):
            st.step(ds.x[:B], ds.y[:B], lens, supports)
        with pytest.raises(ValueError, match=r"sample_weights=.*step\(\) / capture\(\)"):
            st.forward_backward(ds.x[:B], ds.y[:B], lens, supports)
        short = TrainStep(model, task="classification", sample_weights=good_sw[:P - 1].contiguous(), **kw)
        with pytest.raises(ValueError, match=r"sample_weights holds 22 weights, the pool 23 clips"):
            short.forward_backward(ds.x[:B], ds.y[:B], lens, supports, sampler=EpochSampler(P, B, SEED, 0, 1, device=device), label_pool=ds.y)
        s = EpochSampler(P, B, SEED, 0, 1, device=device)
        with pytest.raises(ValueError, match=r"sample_weights holds 22 weights, the pool 23 clips"):
            short.step_from(ds, s, supports)                     # in front of the gather: the cursor has not moved
        assert int(s.cursor.item()) == 0
        with pytest.raises(ValueError, match=r"label pool"):
            st.forward_backward(ds.x[:B], ds.y[:B], lens, supports, sampler=EpochSampler(P, B, SEED, 0, 1, device=device))
        with pytest.raises(ValueError, match=r"quota 4 for class 0, which has 3 clips"):
            BalancedEpochSampler(torch.tensor([0, 0, 0, 1, 1, 1, 1], device=device), 2, SEED, quotas=[4, 1], rank=0, world=1)
        with pytest.raises(ValueError, match=r"batch_size\*world = 4\*2 clips per step, a balanced epoch holds 6"):
            BalancedEpochSampler(torch.tensor([0, 0, 0, 1, 1, 1, 1], device=device), 4, SEED, rank=0, world=2)
        with pytest.raises(ValueError, match=r"labels must be the label pool"):
            BalancedEpochSampler(torch.zeros(4, dtype=torch.int32, device=device), 2, SEED, rank=0, world=1)
        z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
        with pytest.raises(RuntimeError, match=r"cross_entropy: clip_w .* and clip_u .* mutually exclusive"):
            ops.cross_entropy(z(4, 3), z(4, dtype=torch.int64), clip_w=z(4), denom=z(1), clip_u=z(4))
        with pytest.raises(RuntimeError, match=r"bce_with_logits: clip_w .* and clip_u .* mutually exclusive"):
            ops.bce_with_logits(z(4), z(4), clip_w=z(4), denom=z(1), clip_u=z(4))
        with pytest.raises(RuntimeError, match=r"cls_head_loss: clip_w .* and clip_u .* mutually exclusive"):
            ops.cls_head_loss(z(B, N, H), z(1, H), z(1), z(B), "detection", clip_w=z(B), denom=z(1), clip_u=z(B))
        with pytest.raises(RuntimeError, match=r"ce_logits: clip_u must be a float32 tensor of shape \(4,\)"):
            ops.cross_entropy(z(4, 3), z(4, dtype=torch.int64), clip_u=z(3), denom=z(1))
        with pytest.raises(RuntimeError, match=r"clip_weights: sample_w / back belong to the sampler form"):
            ops.clip_weights(z(4), z(4), z(1), sample_w=z(4))
        with pytest.raises(RuntimeError, match=r"clip_weights: class_w must be .* \(2 for float 0 / 1 labels\)"):
            ops.clip_weights(z(4), z(4), z(1), class_w=z(3))
        with pytest.raises(RuntimeError, match=r"clip_weights: norm='mean'"):
            ops.clip_weights(z(4), z(4), z(1), norm="mean")

    assert kernels_run(refusals) == {}, "a refusal was raised behind a launch"
    # the C entry points
    from eeg_gnn_ssl_amd import _lib
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    f4, f1, i4, i1 = z(4), z(1), z(4, dtype=torch.int64), z(1, dtype=torch.int64)
    refused(lib.query("eeg_dcrnn_bce_logits_cw", p(f4), p(f4), 4, None, p(f1), p(f1), p(f4), None), "null clip_u / denom")
    refused(lib.query("eeg_dcrnn_ce_logits_cw", p(f4), p(i4), 1, 4, p(f1), None, p(f1), p(f4), None), "null clip_u / denom")
    cw = lambda *a: lib.query("eeg_dcrnn_clip_weights", *a)     # noqa: E731
    refused(cw(None, 8, None, 0, 0, None, 0, 4, 0, 1, None, 0, None, 0, p(f4), p(f1), None), "null labels")
    refused(cw(p(i4), 2, None, 0, 0, None, 0, 4, 0, 1, None, 0, None, 0, p(f4), p(f1), None), "label_bytes=2")
    refused(cw(p(i4), 8, None, 0, 0, None, 0, 4, 0, 1, None, 0, None, 2, p(f4), p(f1), None), "norm=2")
    refused(cw(p(i4), 8, None, 0, 0, None, 0, 4, 0, 1, p(f4), 0, None, 0, p(f4), p(f1), None), "class_w and C=0 disagree")
    refused(cw(p(f4), 4, None, 0, 0, None, 0, 4, 0, 1, p(f4), 4, None, 0, p(f4), p(f1), None), "float labels are 0 / 1")
    refused(cw(p(i4), 8, p(i4), 4, 4, None, 0, 4, 0, 1, None, 0, None, 0, p(f4), p(f1), None), "perm without cursor")
    refused(cw(p(i4), 8, p(i4), 4, 4, p(i1), 3, 4, 0, 1, None, 0, None, 0, p(f4), p(f1), None), "back=3")
    refused(cw(p(i4), 8, None, 0, 0, None, 0, 4, 0, 1, None, 0, p(f4), 0, p(f4), p(f1), None), "belong to the sampler form")
    refused(cw(p(i4), 8, p(i4), 4, 4, p(i1), 0, 4, 2, 2, None, 0, None, 0, p(f4), p(f1), None), "rank=2, world=2")


# ---- 9. operator registration --------------------------------------------------------------------------------------------------------
def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on the new operators"""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    d = lambda t: t.to(device)     # noqa: E731
    i64 = lambda *v: d(torch.tensor(list(v), dtype=torch.int64))     # noqa: E731
    z, w, bias, y = _head_case(5, 4, device, g)
    clip_u, denom = _weights_of(y, 4, device)
    perm = d(torch.randperm(W_P, generator=g)[:W_LEN])
    samples = [
        (E.cls_head_loss_cw.default, (z, w, bias, y, 1, 0.0, None, clip_u, denom, torch.empty_like(w), torch.empty_like(bias))),
        (E.bce_logits_cw.default, (d(torch.randn(5, generator=g)), d(torch.rand(5, generator=g)), clip_u, denom)),
        (E.ce_logits_cw.default, (d(torch.randn(5, 4, generator=g)), y, clip_u, denom)),
        (E.clip_weights.default, (d(torch.randint(0, 4, (W_P,), generator=g)), perm, i64(12), 8, 1, 2, _f(CLASS_W, device),
                                  d(torch.rand(W_P, generator=g)), 0, d(torch.zeros(4)), d(torch.zeros(1)))),
        (E.clip_weights.default, (d(torch.rand(5, generator=g)), None, None, 0, 0, 1, _f([1.0, POS_W], device), None, 1, d(torch.zeros(5)),
                                  d(torch.zeros(1)))),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
