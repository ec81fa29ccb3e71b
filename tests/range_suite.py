"""Gates, losses and the head where a trained model ends up and no other suite goes: saturated pre-activations, huge logits, exact
ties and exact zeros.  Every other suite draws well-scaled operands (randn inputs, weights of 1 / sqrt(K), biases of 0.1), so the fast
activations of csrc/common.h -- raw v_exp_f32 / v_rcp_f32, correct only if exp2 overflows to +inf, rcp(inf) is 0 and tiny results flush
to 0 -- the three copies of the BCE / cross-entropy arithmetic and the head's arg-max rule are seen at |x| of order 1 only.  Three parts:

A. recurrent and decoder kernels with BANDED biases: the operands, float64 references and drivers of tests/quad_gemm_suite.py and
   tests/dec_kernel_suite.py, with BANDS[i % 13] added to the bias of unit i (reset gate; the update gate rolled by 5, the candidate by
   9; relu cases band the gates only -- a relu candidate with a bias of 1e4 is ill conditioned in fp32, 1.5e-3 on the host).  The table
   crosses both thresholds of the hardware forms: tanh overflows exp2 from x = 44.4, sigmoid from x = 88.7.  One case per kernel
   template that holds an activation; N = 19 / 20 reaches the f32x4 path and the scalar one.
B. the loss kernels (kernels_tail.h plain / _w / _cw, cls_head_loss_body of kernels_head.h, eval_scores_kernel) against float64 torch on
   the same fp32 logits, at |logit| up to 1e4, and the masked loss where its code branches.
C. the head's max over nodes at exact ties and exact zeros: first maximal node, the gradient to that node only, relu'(0) = 0.

Run by tests/test_range.py on the emulator and, marked gpu, on the MI355X.  `python tests/range_suite.py` evaluates the references of
part A in fp32 on the host (must stay below a fifth of every tolerance); `--device cuda|cpu --out FILE` adds the kernels' errors and
writes the table of profiles/range_parity.txt."""
import os
import sys

if __name__ == "__main__":                # (as a script: the paths tests/conftest.py sets up)
    sys.path[1:1] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")]
import numpy as np
import torch
import torch.nn.functional as F

import dec_kernel_suite as dk
import parity_suite as ps
import quad_gemm_suite as qg
import seq_kernel_suite as sk
from oracle import dcrnn_oracle as orc

BANDS = (0.0, 8.0, -8.0, 20.0, -20.0, 45.0, -45.0, 90.0, -90.0, 200.0, -200.0, 1e4, -1e4)
GRAD_TOL = qg.GRAD_TOL
LOSS_TOL, DLOGITS_TOL = 2e-6, 1e-5        # check_training_tail: loss relative to max(1, |ref|), dlogits relative to their maximum
ROW_SUM_TOL = 1e-6                        # a cross-entropy gradient row sums to 0 within this / B


def band(h):
    """unit i -> BANDS[i % 13]"""
    return torch.tensor(BANDS)[torch.arange(h) % len(BANDS)]


def gate_band(h):
    return torch.cat([band(h), band(h).roll(5)])          # [reset | update]


def cand_band(h):
    return band(h).roll(9)


def _leaf(t, device):
    """a leaf of its own on `device` (on the CPU `.to` hands back the tensor itself)"""
    return t.detach().clone().to(device).requires_grad_(True)


def _leaf64(t):
    return t.detach().double().clone().requires_grad_(True)


def _finite(t):
    return bool(torch.isfinite(torch.as_tensor(t)).all())


def assert_yardstick(yard, out_key, what):
    """the project's standing rule: the reference's own arithmetic in fp32 on the host stays below a fifth of every tolerance, else the
    operands -- not a kernel -- are what a failure would measure"""
    for k, v in yard.items():
        tol = ps.TOL if k == out_key else GRAD_TOL
        assert v < 0.2 * tol, f"{what}: fp32 host yardstick of {k} is {v:.2e}, not below a fifth of {tol:.0e}: badly scaled operands"


# ---- A. one DCGRU layer with banded biases ---------------------------------------------------------------------------------------
# kernel template -> cases of tests/seq_kernel_suite.py (their shapes, supports and expected kernels)
LAYER_CASES = ("h16_m3_n19", "h32_m2_n20",          # one-wave, N <= 20
               "h64_m2_n32", "h64_m3_n31_walk",     # one-wave, N > 20 (NKS = 8): relu / tanh
               "h64_m5_n20",                        # one-wave, M = 5 (relu: gates only)
               "h64_m3_n19",                        # two-wave
               "h64_m3_n20_spec",                   # two-wave SPEC
               "h64_m4_b384")                       # streamed BPTT
# the emulator's share: clip counts of at most 5; the streamed BPTT kernel under dev knob 3 (sk.KNOB_CASES, on the two-wave case)
EMU_LAYER_CASES = ("h16_m3_n19", "h32_m2_n20", "h64_m2_n32", "h64_m5_n20", "h64_m3_n19", "h64_m3_n20_spec")
EMU_KNOB_LAYER_CASES = ("stream_m3",)

_LAYER_REF = {}


def layer_operands(case, seed=0):
    op = qg.make_operands(case, case["t"], case["b"], seed)
    op["bg"] = op["bg"] + gate_band(case["h"])
    if case["act"] == "tanh":
        op["bc"] = op["bc"] + cand_band(case["h"])
    return op


def layer_reference(name, seed=0):
    """(operands, cotangent, float64 hseq, float64 gradients, fp32 host yardstick) of a case, computed once per process"""
    key = (name, seed)
    if key not in _LAYER_REF:
        case = sk.CASES[name]
        op = layer_operands(case, seed)
        cot = (op["w"], op["wsel"])
        hseq, grads = qg.reference(case, op, [cot])
        op32 = {k: v.clone() if torch.is_tensor(v) else v for k, v in op.items()}          # (its leaves are the fp32 tensors themselves)
        h32, g32 = qg.reference(case, op32, [cot], dtype=torch.float32)
        g32 = {k: g for k, g in g32[0].items() if k != "dh0" or case["h0"]}
        _LAYER_REF[key] = (op, cot, hseq, grads[0], sk.errors(h32, g32, hseq, grads[0]))
    return _LAYER_REF[key]


def check_layer(name, device, expect=None, seed=0, report=None):
    """One banded layer on `device`: the expected recurrent kernels ran (event recorder), hseq under assert_close at TOL, every gradient
    under assert_close_scaled at GRAD_TOL, everything finite, and -- tanh -- |hseq| <= max(1, max |h0|) (1 + 1e-6): the state is a
    convex combination of its previous value and a tanh.  expect: the kernels under dev knobs (sk.KNOB_CASES)."""
    case = sk.CASES[name]
    op, cot, ref_hseq, ref_grads, yard = layer_reference(name, seed)
    what = f"range {name} T={case['t']} B={case['b']} N={case['n']}"
    assert_yardstick(yard, "hseq", what)
    run = qg.run_layer(case, op, *cot, device)
    run()                                                                                 # (first call: allocations)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=run()))
    hseq, grads = out["res"]
    sk.assert_ran(ran, expect if expect is not None else case["expect"], what)
    if case["spectral"]:
        assert "gemm_nn_xw" in ran and ("spec_mix_y" in ran) == (not case["expect"]["seq_fwd"].endswith("true>")), f"{what}: {sorted(ran)}"
    errs = sk.errors(hseq, grads, ref_hseq, ref_grads)
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"{what} ran: " + "; ".join(f"{role} = {sym}" for role in ("seq_fwd", "seq_bwd") for sym in ran.get(role, {})))
    if report is not None:
        report[name] = (yard, errs)
    assert _finite(hseq) and all(_finite(g) for g in grads.values()), f"{what}: a non-finite value in {[k for k, g in grads.items() if not _finite(g)] or 'hseq'}"
    ps.assert_close(hseq.cpu().numpy(), ref_hseq.numpy(), f"{what}: hseq")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
    if case["act"] == "tanh":
        bound = max(1.0, float(op["h0"].abs().max()) if op["h0"] is not None else 0.0) * (1 + 1e-6)
        assert float(hseq.abs().max()) <= bound, f"{what}: |hseq| reaches {float(hseq.abs().max()):.9g}, beyond {bound:.9g}"
    return errs


# ---- A. the persistent decoder with banded biases ----------------------------------------------------------------------------------
# narrow outputs (tanh, 1 / 2 / 4 layers) and a first layer wider than 128 outputs, which takes the wide backward (relu: gates only)
DEC_CASES = ("m1_d48_l1", "m2_d112_l2", "m3_d64_l4", "m3_d160_l4")
EMU_DEC_CASES = ("m1_d48_l1", "m3_d64_l4", "m3_d160_l4")

_DEC_REF = {}


def decoder_operands(case, seed=0):
    """dk.make_operands (a fresh set: nothing of that suite's cache is touched) with the bands on every cell's biases; the layers
    from 1 on share one cell, whose tensors are banded once"""
    op = dk.make_operands(case, seed)
    done = set()
    for k, v in op["params"].items():
        if not k.endswith(".biases") or v.data_ptr() in done:
            continue
        done.add(v.data_ptr())
        if "dconv_gate" in k:
            v.add_(gate_band(dk.H))
        elif case["act"] == "tanh":
            v.add_(cand_band(dk.H))
    return op


def decoder_reference(name, seed=0):
    key = (name, seed)
    if key not in _DEC_REF:
        case = dk.CASES[name]
        op = decoder_operands(case, seed)
        out, grads = dk.reference(case, op, [op["wout"]])
        o32, g32 = dk.reference(case, op, [op["wout"]], dtype=torch.float32)
        _DEC_REF[key] = (op, out, grads[0], dk.errors(o32, g32[0], out, grads[0]))
    return _DEC_REF[key]


def check_decoder(name, device, seed=0, report=None):
    """One banded decoder on `device`: the expected persistent kernels ran and no per-step launch, outputs under assert_close at TOL,
    dh0 and every parameter gradient under assert_close_scaled at GRAD_TOL, everything finite"""
    from eeg_gnn_ssl_amd import ops
    case = dk.CASES[name]
    assert ops.decoder_is_persistent(case["t"], case["b"], case["n"], dk.H, case["dout"], case["m"], case["layers"]), name
    op, ref_out, ref_grads, yard = decoder_reference(name, seed)
    what = f"range {name} T={case['t']} B={case['b']} N={case['n']}"
    assert_yardstick(yard, "out", what)
    run = dk.run_decoder(case, op, op["wout"], device)
    if device != "cpu":
        run()                                                                             # (first call: allocations)
    res = {}
    ran = ps.kernels_run(lambda: res.update(res=run()))
    out, grads = res["res"]
    dk.assert_ran(ran, case, what)
    errs = dk.errors(out, grads, ref_out, ref_grads)
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"{what} ran: " + "; ".join(f"{role} = {sym}" for role in ("dec_fwd_persist", "dec_bwd_persist") for sym in ran.get(role, {})))
    if report is not None:
        report[name] = (yard, errs)
    assert set(grads) == set(ref_grads), (sorted(grads), sorted(ref_grads))
    assert _finite(out) and all(_finite(g) for g in grads.values()), f"{what}: a non-finite value in {[k for k, g in grads.items() if not _finite(g)] or 'outputs'}"
    ps.assert_close(out.cpu().numpy(), ref_out.numpy(), f"{what}: outputs")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
    return errs


# ---- B. the criteria against float64 torch on the same fp32 logits -------------------------------------------------------------------
BCE_LOGITS = (0.0,) + tuple(s * v for v in (1e-8, 1e-3, 1.0, 16.5, 17.5, 20.0, 87.0, 88.5, 89.5, 104.0, 1e4) for s in (1.0, -1.0))
BCE_TARGETS = (0.0, 1.0, 0.3)
FORMS = ("plain", "clip_w", "clip_u")


def bce_set(tiles=1):
    """every logit x every target (B = 69), tiled (5 tiles: B = 345, across the 256-thread stride of the single workgroup)"""
    x = torch.tensor([v for v in BCE_LOGITS for _ in BCE_TARGETS])
    y = torch.tensor([t for _ in BCE_LOGITS for t in BCE_TARGETS])
    return x.repeat(tiles), y.repeat(tiles)


def ce_set(c, tiles=1):
    """rows of C logits x targets at the largest and at the smallest logit (all entries equal: the first and the last class):
    [0, 200, -200, 1e4]-style spreads, all entries equal (small, moderate, huge), a spread of 100 (around 0 and on top of 900)"""
    base = torch.tensor([0.0, 200.0, -200.0, 1e4, -1e4, 88.5, -104.0])
    rows = [base[:c], base[:c].flip(0), base[7 - c:], 1e4 * F.one_hot(torch.tensor(c - 1), c).float(), -1e4 * F.one_hot(torch.tensor(0), c).float()]
    rows += [torch.full((c,), v) for v in (0.0, 17.5, 88.5, 1e4, -1e4)]
    rows += [torch.linspace(-50.0, 50.0, c), torch.linspace(1000.0, 900.0, c)]
    x, y = [], []
    for r in rows:
        hi, lo = int(r.argmax()), int(r.argmin())
        for t in ((hi, lo) if hi != lo else (0, c - 1)):
            x.append(r)
            y.append(t)
    return torch.stack(x).repeat(tiles, 1), torch.tensor(y, dtype=torch.int64).repeat(tiles)


def clip_weights_for(form, b, sum_norm):
    """-> (multiplier per clip as the float64 reference applies it, keyword arguments of the operator).  clip_w: zeros and ones, the
    mean over the clips that count; clip_u: multipliers in {0, 0.5, 3}, divided by their sum (nn.CrossEntropyLoss(weight=)) or by B
    (nn.BCEWithLogitsLoss(pos_weight=)).  The patterns have periods coprime to the 3 targets and 2 labels per logit row."""
    i = torch.arange(b)
    if form == "plain":
        return torch.ones(b), float(b), {}
    if form == "clip_w":
        w = ((i + i // 69) % 4 != 1).float()
        return w, float(w.sum()), dict(clip_w=w, denom=w.sum().view(1))
    u = torch.tensor([0.0, 0.5, 3.0])[(i + i // 3 + i // 69) % 3]
    denom = u.sum().view(1) if sum_norm else torch.tensor([float(b)])
    return u, float(denom), dict(clip_u=u, denom=denom)


def ref_criterion(kind, x, y, u, denom):
    """float64 torch on the fp32 logits: sum_b u_b * l_b / denom and its gradient; per-clip terms l_b as well"""
    xd = _leaf64(x)
    terms = F.binary_cross_entropy_with_logits(xd, y.double(), reduction="none") if kind == "bce" else F.cross_entropy(xd, y, reduction="none")
    loss = (u.double() * terms).sum() / denom
    loss.backward()
    return float(loss.detach()), xd.grad, terms.detach()


def _on(device, kw):
    return {k: v.to(device) for k, v in kw.items()}


def assert_criterion(what, loss, dx, ref_loss, ref_dx, u, b, ce):
    print(f"range {what}: loss {loss:.9g} ref {ref_loss:.9g} err/scale {abs(loss - ref_loss) / max(1.0, abs(ref_loss)):.2e}  dlogits "
          f"{float((dx.double() - ref_dx).abs().max() / ref_dx.abs().max().clamp_min(1e-6)):.2e}"
          + (f"  row sums * B {float(dx.double().sum(1).abs().max()) * b:.2e}" if ce else ""))
    assert np.isfinite(loss) and _finite(dx), f"{what}: non-finite loss or gradient"
    assert abs(loss - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss)), f"{what}: loss {loss!r}, float64 {ref_loss!r}"
    ps.assert_close_scaled(dx.numpy(), ref_dx.numpy(), f"{what}: dlogits", tol=DLOGITS_TOL)
    assert not dx[u == 0].any(), f"{what}: a clip that does not count has a gradient"
    if ce:
        worst = float(dx.double().sum(1).abs().max())
        assert worst <= ROW_SUM_TOL / b, f"{what}: a gradient row sums to {worst:.3e}, beyond {ROW_SUM_TOL / b:.3e}"


def check_bce(device, report=None):
    """ops.bce_with_logits plain, with clip_w and with clip_u at B = 69 and B = 345"""
    from eeg_gnn_ssl_amd import ops
    for tiles in (1, 5):
        x, y = bce_set(tiles)
        b = x.numel()
        for form in FORMS:
            u, denom, kw = clip_weights_for(form, b, sum_norm=False)
            ref_loss, ref_dx, _ = ref_criterion("bce", x, y, u, denom)
            xd = _leaf(x, device)
            loss = ops.bce_with_logits(xd, y.to(device), **_on(device, kw))
            loss.backward()
            what = f"bce {form} B={b}"
            assert_criterion(what, float(loss.detach()), xd.grad.cpu(), ref_loss, ref_dx, u, b, ce=False)
            if report is not None:
                report[what] = dict(loss=abs(float(loss.detach()) - ref_loss) / max(1.0, abs(ref_loss)),
                                    dlogits=float((xd.grad.cpu().double() - ref_dx).abs().max() / ref_dx.abs().max()))


def check_ce(device, report=None):
    """ops.cross_entropy plain, with clip_w and with clip_u at C = 2, 4, 7; the row set once and tiled beyond 256 clips"""
    from eeg_gnn_ssl_amd import ops
    for c in (2, 4, 7):
        for tiles in (1, 14):
            x, y = ce_set(c, tiles)
            b = x.shape[0]
            assert tiles == 1 or b > 256
            for form in FORMS:
                u, denom, kw = clip_weights_for(form, b, sum_norm=True)
                ref_loss, ref_dx, _ = ref_criterion("ce", x, y, u, denom)
                xd = _leaf(x, device)
                loss = ops.cross_entropy(xd, y.to(device), **_on(device, kw))
                loss.backward()
                what = f"ce {form} C={c} B={b}"
                assert_criterion(what, float(loss.detach()), xd.grad.cpu(), ref_loss, ref_dx, u, b, ce=True)
                if report is not None:
                    report[what] = dict(loss=abs(float(loss.detach()) - ref_loss) / max(1.0, abs(ref_loss)),
                                        dlogits=float((xd.grad.cpu().double() - ref_dx).abs().max() / ref_dx.abs().max()),
                                        row_sum_x_B=float(xd.grad.cpu().double().sum(1).abs().max()) * b)


def head_operands(x):
    """(z, W, bias) of a head with N = 1 whose logits are x (B, C) exactly: z >= 0 holds max(x, 0) and max(-x, 0) in two units per
    class, W their +1 / -1, bias 0 -- every product is exact and one of the two terms is 0"""
    b, c = x.shape
    h = (2 * c + 3) // 4 * 4
    z = torch.zeros(b, 1, h)
    z[:, 0, 0:2 * c:2] = x.clamp_min(0)
    z[:, 0, 1:2 * c:2] = (-x).clamp_min(0)
    w = torch.zeros(c, h)
    w[torch.arange(c), 2 * torch.arange(c)] = 1.0
    w[torch.arange(c), 2 * torch.arange(c) + 1] = -1.0
    return z, w, torch.zeros(c)


def check_head_criteria(device, report=None):
    """the same logit and target sets through ops.cls_head_loss (cls_head_loss_body: the third copy of the arithmetic), N = 1 and an
    identity-like fc: logits are returned bit for bit, the loss is the criterion, dbias the batch sum of dlogits and dz carries
    +dlogits / -dlogits at the one unit of a class that is not 0"""
    from eeg_gnn_ssl_amd import ops
    sets = [("bce", 1, bce_set(t)) for t in (1, 5)] + [("ce", c, ce_set(c, t)) for c in (2, 4, 7) for t in (1, 14)]
    for kind, c, (x, y) in sets:
        b = x.shape[0]
        x2 = x.view(b, c)
        z, w, bias = head_operands(x2)
        for form in FORMS:
            u, denom, kw = clip_weights_for(form, b, sum_norm=kind == "ce")
            ref_loss, ref_dx, _ = ref_criterion(kind, x, y, u, denom)
            ref_dx = ref_dx.view(b, c)
            wd, bd = _leaf(w, device), _leaf(bias, device)
            loss, logits, dz = ops.cls_head_loss(z.to(device), wd, bd, y.to(device), "detection" if kind == "bce" else "classification", **_on(device, kw))
            what = f"head {kind} {form} C={c} B={b}"
            loss, dz, db = float(loss.detach()), dz.cpu(), bd.grad.cpu()
            assert torch.equal(logits.cpu(), x2), f"{what}: the head's logits are not the constructed ones"
            # dlogits as the head's backward spread them: at the unit that holds |x| (x == 0: both units are 0 and so is dz)
            dl = dz[:, 0, 0:2 * c:2] - dz[:, 0, 1:2 * c:2]
            want = torch.where(x2 != 0, ref_dx, torch.zeros_like(ref_dx))
            e_loss = abs(loss - ref_loss) / max(1.0, abs(ref_loss))
            e_dl = float((dl.double() - want).abs().max() / want.abs().max().clamp_min(1e-6))
            e_db = float((db.double() - ref_dx.sum(0)).abs().max() / max(1e-3, float(ref_dx.sum(0).abs().max())))
            print(f"range {what}: loss {e_loss:.2e} dlogits (from dz) {e_dl:.2e} dbias {e_db:.2e}")
            if report is not None:
                report[what] = dict(loss=e_loss, dlogits=e_dl, dbias=e_db)
            assert np.isfinite(loss) and _finite(dz) and _finite(db) and _finite(wd.grad), f"{what}: a non-finite value"
            assert e_loss <= LOSS_TOL, f"{what}: loss {loss!r}, float64 {ref_loss!r}"
            ps.assert_close_scaled(dl.numpy(), want.numpy(), f"{what}: dlogits read from dz", tol=DLOGITS_TOL)
            assert e_db <= LOSS_TOL, f"{what}: dbias differs from the float64 batch sum by {e_db:.3e} of its maximum"   # (check_cls_head_loss: 2e-6 of max(1e-3, max))
            assert not dz[u == 0].any(), f"{what}: a clip that does not count has a gradient"


def check_eval_scores(device, report=None):
    """ops.eval_scores on the same sets: the per-clip loss is bit for bit the training criterion of that clip as a batch of one
    (kernels_eval.h documents it), and loss and probabilities agree with float64.  Probabilities: 1e-6 absolute -- values in [0, 1]
    from one or two expf of a few ulp each (2.4e-7) and one division."""
    from eeg_gnn_ssl_amd import ops
    for kind, c, (x, y) in [("bce", 1, bce_set())] + [("ce", c, ce_set(c)) for c in (2, 4, 7)]:
        b = x.shape[0]
        xd = x.view(b, c).to(device).contiguous()
        pool = y.to(device)
        probs = torch.full((b,) if c == 1 else (b, c), -1.0, device=device)
        losses = torch.full((b,), -1.0, device=device)
        ops.eval_scores(xd, pool, torch.ones(b, device=device), torch.tensor([b], dtype=torch.int64, device=device), probs, losses)
        _, _, terms = ref_criterion(kind, x, y, torch.ones(b), float(b))
        ref_p = torch.sigmoid(x.double()) if c == 1 else torch.softmax(x.double(), 1)
        fn = ops.bce_with_logits if kind == "bce" else ops.cross_entropy
        train = torch.stack([fn(xd[i] if c == 1 else xd[i:i + 1], pool[i:i + 1]) for i in range(b)]).cpu()
        losses, probs = losses.cpu(), probs.cpu()
        what = f"eval {kind} C={c} B={b}"
        e_l = float(((losses.double() - terms).abs() / terms.abs().clamp_min(1.0)).max())
        e_p = float((probs.double() - ref_p).abs().max())
        print(f"range {what}: per-clip loss {e_l:.2e} probs {e_p:.2e}")
        if report is not None:
            report[what] = dict(loss=e_l, probs=e_p)
        assert _finite(losses) and _finite(probs), f"{what}: a non-finite score"
        assert torch.equal(losses, train), f"{what}: a clip's evaluation loss is not the bits of its training term, first at clip {int((losses != train).nonzero()[0])}"
        assert e_l <= LOSS_TOL, f"{what}: a per-clip loss is {e_l:.3e} from float64 (relative to max(1, |ref|))"
        assert e_p <= 1e-6, f"{what}: a probability is {e_p:.3e} from float64"


def check_masked_loss_edges(device):
    """ops.masked_regression_loss where the finish kernel branches: no counted element (every element masked; every clip_w zero) ->
    loss 0 and a gradient of exact zeros; a masked RMSE of 0 (pred == y) -> loss 0 and gradient 0, the kernel's documented convention
    (kernels_tail.h, masked_loss_finish_body) -- the oracle divides 0 by 0 there and returns a NaN gradient, checked below, so the
    convention is what is asserted; and n = 1, 3, 4, 5 elements, which the tail path of the last thread takes alone (n < 4) or after
    one 16-byte piece, against the float64 oracle at the tolerances of check_training_tail."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(31)

    def run(pred, y, name, **kw):
        pd = _leaf(pred, device)
        loss = ops.masked_regression_loss(pd, y.to(device), None, None, name, **_on(device, kw))
        loss.backward()
        return float(loss.detach()), pd.grad.cpu()

    for name in ("mae", "rmse"):
        for shape in ((7,), (4, 9)):
            pred = torch.randn(shape, generator=g)
            loss, grad = run(pred, torch.zeros(shape), name)                              # y == mask_val everywhere
            assert loss == 0.0 and not grad.any(), (name, shape, "all masked", loss)
        pred, y = torch.randn(4, 9, generator=g), torch.randn(4, 9, generator=g)
        loss, grad = run(pred, y, name, clip_w=torch.zeros(4), denom=torch.ones(1))
        assert loss == 0.0 and not grad.any(), (name, "every clip_w zero", loss)
    y = torch.randn(3, 10, generator=g)
    loss, grad = run(y, y, "rmse")
    assert loss == 0.0 and not grad.any(), ("rmse of 0", loss)
    po = _leaf64(y)
    orc.regression_loss(y.double(), po, None, None, "rmse").backward()
    assert bool(torch.isnan(po.grad).all())                                               # (the oracle: d sqrt at 0 times 0)
    loss, grad = run(y, y, "rmse", clip_w=torch.tensor([1.0, 0.0, 1.0]), denom=torch.tensor([2.0]))
    assert loss == 0.0 and not grad.any(), ("weighted rmse of 0", loss)
    for n in (1, 3, 4, 5):
        pred, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
        if n >= 3:
            y[1] = 0.0                                                                    # (one masked element)
        w = torch.ones(n)
        w[n // 2] = 0.0                                                                   # (n = 1: the one clip does not count -> 0)
        for name in ("mae", "rmse"):
            for weighted in (False, True):
                keep = (w != 0) if weighted else torch.ones(n, dtype=torch.bool)
                kw = dict(clip_w=w, denom=w.sum().clamp_min(1.0).view(1)) if weighted else {}
                loss, grad = run(pred, y, name, **kw)
                what = f"masked {name} n={n}{' weighted' if weighted else ''}"
                if not bool((keep & (y != 0)).any()):
                    assert loss == 0.0 and not grad.any(), what
                    continue
                po = _leaf64(pred)
                ref = orc.regression_loss(y.double()[keep], po[keep], None, None, name)
                ref.backward()
                ref = float(ref.detach())
                assert abs(loss - ref) <= LOSS_TOL * max(1.0, abs(ref)), (what, loss, ref)
                ps.assert_close_scaled(grad.numpy(), po.grad.numpy(), f"{what}: dpred", tol=DLOGITS_TOL)
                assert not grad[~(keep & (y != 0))].any(), what


# ---- C. the head at ties and zeros ----------------------------------------------------------------------------------------------
HEAD_SHAPES = ((19, 64, 1), (19, 64, 4), (21, 32, 3))
TIE_K, TIE_J = 4, 11
CONSTRUCTIONS = ("a", "b", "c", "d")


def head_tie_operands(n, h, c, seed=0):
    """B = 8: the four constructions twice with other values (the second half meets the zero weights of the clip_w / clip_u forms).
    W = |W| (construction (c) needs it; the others do not mind), so that a node row of positive z beats the bias alone.
      (a) all node rows identical: every node ties on every class;
      (b) z <= 0 everywhere, zeros among the negatives: relu leaves nothing, every node's logit is the bias;
      (c) rows TIE_K = 4 and TIE_J = 11 identical and positive, every other row negative: the two tie above the rest;
      (d) as (c) with some entries of the two rows exactly 0."""
    g = torch.Generator().manual_seed(seed)
    w = (0.05 * torch.randn(c, h, generator=g)).abs()        # (logits of a positive row stay near 2: their fp32 rounding, which a softmax passes on, stays a tenth of the bounds)
    bias = 0.1 * torch.randn(c, generator=g)
    z = torch.empty(8, n, h)
    zero_at = torch.zeros(8, h, dtype=torch.bool)
    for i in range(8):
        kind = CONSTRUCTIONS[i % 4]
        row = torch.randn(h, generator=g)
        if kind == "a":
            z[i] = row                                        # (mixed signs: relu'(negative) = 0 on the winning row too)
        elif kind == "b":
            z[i] = -torch.rand(n, h, generator=g)
            z[i][torch.rand(n, h, generator=g) < 0.25] = 0.0
        else:
            z[i] = -0.1 - torch.rand(n, h, generator=g)
            row = 0.1 + row.abs()
            if kind == "d":
                zero_at[i] = torch.rand(h, generator=g) < 0.3
                zero_at[i, 0] = True
                row[zero_at[i]] = 0.0
            z[i, TIE_K] = row
            z[i, TIE_J] = row
    return z, w, bias, zero_at


def tie_weights(form, sum_norm):
    """as clip_weights_for, for the 8 clips of head_tie_operands: every construction counts in the first half, the zeros sit in the second"""
    if form == "plain":
        return torch.ones(8), 8.0, {}
    if form == "clip_w":
        w = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0])
        return w, float(w.sum()), dict(clip_w=w, denom=w.sum().view(1))
    u = torch.tensor([0.5, 3.0, 0.5, 3.0, 0.0, 3.0, 0.5, 0.0])
    denom = u.sum().view(1) if sum_norm else torch.tensor([8.0])
    return u, float(denom), dict(clip_u=u, denom=denom)


def ref_head(z, w, bias, y, kind, u, denom):
    """float64: relu(z) @ W.T + b, .max(dim=1), the criterion -> everything the head returns.  torch's max takes the first maximal
    index and sends the gradient to that index alone, and relu'(0) = 0"""
    zd, wd, bd = (_leaf64(t) for t in (z, w, bias))
    nl = torch.relu(zd) @ wd.t() + bd
    logits, arg = nl.max(dim=1)
    logits.retain_grad()
    yy = y.double().view(-1, 1) if kind == "bce" else y
    terms = F.binary_cross_entropy_with_logits(logits, yy, reduction="none").view(-1) if kind == "bce" else F.cross_entropy(logits, yy, reduction="none")
    loss = (u.double() * terms).sum() / denom
    loss.backward()
    return dict(logits=logits.detach(), arg=arg, loss=float(loss.detach()), dlogits=logits.grad, dz=zd.grad, dW=wd.grad, db=bd.grad)


def assert_tie_pattern(what, z, arg, dz, dl, bias, logits, zero_at):
    """what is exact: the winning node, where dz may be anything but zero, and the logits of the dead clips"""
    b, n, h = z.shape
    c = arg.shape[1]
    for i in range(b):
        kind = CONSTRUCTIONS[i % 4]
        want = 0 if kind in ("a", "b") else TIE_K
        assert arg[i].tolist() == [want] * c, f"{what}: clip {i} ({kind}) takes node {arg[i].tolist()}, the first maximal one is {want}"
        others = [q for q in range(n) if q != want]
        assert not dz[i, others].any(), f"{what}: clip {i} ({kind}) has a gradient on a node that is not the first maximal one"
        if kind == "b":
            assert torch.equal(logits[i], bias), f"{what}: clip {i} (b): logits {logits[i].tolist()} are not the bias {bias.tolist()}"
            assert not dz[i].any(), f"{what}: clip {i} (b): dz is not zero behind a relu of z <= 0"
        if kind == "a":
            assert not dz[i, 0][z[i, 0] <= 0].any(), f"{what}: clip {i} (a): a gradient where z <= 0"
        if kind == "d":
            assert zero_at[i].any() and not dz[i, TIE_K][zero_at[i]].any(), f"{what}: clip {i} (d): dz is not exactly 0 where z is exactly 0"
        if kind in ("c", "d") and dl[i].any():
            assert dz[i, TIE_K][~zero_at[i]].any(), f"{what}: clip {i} ({kind}): the winning row has no gradient"


def check_head_ties(device, report=None):
    """ops.cls_head under autograd and ops.cls_head_loss (plain, clip_w, clip_u) on the four constructions: `arg` and the zero
    pattern exact; logits, loss, dz, dW, dbias against float64 at the tolerances of check_cls_head_loss (2e-6 of max(1, |ref|) for
    the loss and, of max(1e-3, max |ref|), for the gradients of fc; dz likewise)."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(3)

    def close(got, ref, what, floor=1e-3):
        e = float((got.double() - ref).abs().max()) / max(floor, float(ref.abs().max()))
        assert e <= LOSS_TOL, f"{what}: {e:.3e} of the maximum from float64"
        return e

    for n, h, c in HEAD_SHAPES:
        z, w, bias, zero_at = head_tie_operands(n, h, c)
        b = z.shape[0]
        kind = "bce" if c == 1 else "ce"
        y = (torch.rand(b, generator=g) > 0.5).float() if c == 1 else torch.randint(0, c, (b,), generator=g)
        # ---- ops.cls_head with autograd: a cotangent of our own stands for the criterion
        cot = torch.randn(b, c, generator=g)
        zd, wd, bd = (_leaf(t, device) for t in (z, w, bias))
        logits, arg = torch.ops.eeg_dcrnn.cls_head(zd, wd, bd, 0.0, None)
        assert torch.equal(ops.cls_head(zd, wd, bd), logits)
        logits.backward(cot.to(device))
        zr, wr, br = (_leaf64(t) for t in (z, w, bias))
        ref_logits, ref_arg = (torch.relu(zr) @ wr.t() + br).max(dim=1)
        ref_logits.backward(cot.double())
        what = f"head ties cls_head N={n} H={h} C={c}"
        assert torch.equal(ref_arg, arg.cpu().long()), f"{what}: arg {arg.cpu().tolist()}, torch's {ref_arg.tolist()}"
        assert_tie_pattern(what, z, arg.cpu(), zd.grad.cpu(), cot, bias, logits.detach().cpu(), zero_at)
        errs = dict(logits=close(logits.detach().cpu(), ref_logits.detach(), f"{what}: logits", floor=1.0),
                    dz=close(zd.grad.cpu(), zr.grad, f"{what}: dz"), dW=close(wd.grad.cpu(), wr.grad, f"{what}: dW"),
                    db=close(bd.grad.cpu(), br.grad, f"{what}: dbias"))
        dead = [i for i in range(b) if CONSTRUCTIONS[i % 4] == "b"]
        print(f"range {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        if report is not None:
            report[what] = errs
        # ---- ops.cls_head_loss in its three forms
        for form in FORMS:
            u, denom, kw = tie_weights(form, sum_norm=c > 1)
            ref = ref_head(z, w, bias, y, kind, u, denom)
            wd, bd = _leaf(w, device), _leaf(bias, device)
            loss, logits, _arg, dl, dz = _cls_head_loss_op(form)(z.to(device), wd, bd, y.to(device), kind, kw, device)
            what = f"head ties cls_head_loss {form} N={n} H={h} C={c}"
            arg, dz, dl, logits = _arg.cpu(), dz.cpu(), dl.cpu(), logits.cpu()
            assert torch.equal(ref["arg"], arg.long()), f"{what}: arg {arg.tolist()}, torch's {ref['arg'].tolist()}"
            assert_tie_pattern(what, z, arg, dz, dl, bias, logits, zero_at)
            assert not dz[u == 0].any() and not dl[u == 0].any(), f"{what}: a clip that does not count has a gradient"
            errs = dict(loss=abs(loss - ref["loss"]) / max(1.0, abs(ref["loss"])),
                        logits=close(logits, ref["logits"], f"{what}: logits", floor=1.0), dz=close(dz, ref["dz"], f"{what}: dz"),
                        dW=close(wd.grad.cpu(), ref["dW"], f"{what}: dW"), db=close(bd.grad.cpu(), ref["db"], f"{what}: dbias"))
            print(f"range {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            if report is not None:
                report[what] = errs
            assert errs["loss"] <= LOSS_TOL, f"{what}: loss {loss!r}, float64 {ref['loss']!r}"
            ps.assert_close_scaled(dl.numpy(), ref["dlogits"].numpy(), f"{what}: dlogits", tol=DLOGITS_TOL)
            # (b): dW gets nothing from a dead clip and dbias all of its dlogits -- with the dead clips alone in the batch, exactly
            if form == "plain":
                zb, yb = z[dead], y[dead]
                wd, bd = _leaf(w, device), _leaf(bias, device)
                _, _, _, dlb, dzb = _cls_head_loss_op(form)(zb.to(device), wd, bd, yb.to(device), kind, {}, device)
                assert not dzb.any() and not wd.grad.any(), f"{what}: dz / dW of clips with z <= 0 are not exactly zero"
                close(bd.grad.cpu(), dlb.cpu().double().sum(0), f"{what}: dbias of the dead clips against the sum of their dlogits")


def _cls_head_loss_op(form):
    """ops.cls_head_loss, and behind it the operator once more for what the public function does not return (arg, dlogits): same
    kernels, same bits -- asserted"""
    from eeg_gnn_ssl_amd import ops

    def call(z, w, bias, y, kind, kw, device):
        kw = _on(device, kw)
        loss, logits, dz = ops.cls_head_loss(z, w, bias, y, "detection" if kind == "bce" else "classification", **kw)
        k = 0 if kind == "bce" else 1
        scratch = (torch.empty_like(w), torch.empty_like(bias))
        if form == "plain":
            res = torch.ops.eeg_dcrnn.cls_head_loss(z, w.detach(), bias.detach(), y, k, 0.0, None, *scratch)
        elif form == "clip_w":
            res = torch.ops.eeg_dcrnn.cls_head_loss_w(z, w.detach(), bias.detach(), y, k, 0.0, None, kw["clip_w"], kw["denom"], *scratch)
        else:
            res = torch.ops.eeg_dcrnn.cls_head_loss_cw(z, w.detach(), bias.detach(), y, k, 0.0, None, kw["clip_u"], kw["denom"], *scratch)
        loss2, logits2, arg, dl, dz2 = res
        assert float(loss2[0]) == float(loss.detach()) and torch.equal(logits2, logits) and torch.equal(dz2, dz)
        return float(loss.detach()), logits, arg, dl, dz
    return call


# ---- yardstick and parity table -------------------------------------------------------------------------------------------------
def _fractions(errs, out_key):
    return errs[out_key] / ps.TOL, max(v for k, v in errs.items() if k != out_key) / GRAD_TOL


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[-1])
    ap.add_argument("--device", choices=("cuda", "cpu"))
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    torch.set_num_threads(16)
    emu = None
    if a.device == "cpu":
        import emu_support
        emu = emu_support.install_emulator()
    where = {"cuda": "MI355X", "cpu": "emulator", None: ""}[a.device]
    lines = [f"{'A. banded biases (errors as fractions of tolerance)':<56}{'out':>9}{'grads':>9}  worst gradient"]
    worst = 0.0
    layers = [(n, None) for n in (EMU_LAYER_CASES if a.device == "cpu" else LAYER_CASES)] + ([(n, n) for n in EMU_KNOB_LAYER_CASES] if emu else [])
    decoders = EMU_DEC_CASES if a.device == "cpu" else DEC_CASES
    for out_key, names in (("hseq", layers), ("out", [(n, None) for n in decoders])):
        for name, knob in names:
            base, knobs, expect = sk.KNOB_CASES[knob] if knob else (name, {}, None)
            yard = (layer_reference(base) if out_key == "hseq" else decoder_reference(base))[-1]
            rows = [(f"{knob or name}  fp32 host", yard)]
            worst = max(worst, *_fractions(yard, out_key))
            if a.device:
                rep = {}
                for key, value in knobs.items():
                    emu.call("eeg_dcrnn_set_tuning", key, value)
                try:
                    check_layer(base, a.device, expect=expect, report=rep) if out_key == "hseq" else check_decoder(base, a.device, report=rep)
                finally:
                    for key in knobs:
                        emu.call("eeg_dcrnn_set_tuning", key, 0)
                rows.append((f"{'':<{len(knob or name)}}  {where}", rep[base][1]))
            for label, errs in rows:
                o, g = _fractions(errs, out_key)
                lines.append(f"{label:<56}{o:>9.3f}{g:>9.3f}  {max((k for k in errs if k != out_key), key=lambda k: errs[k])}")
            print("\n".join(lines[-len(rows):]), flush=True)
    lines.append(f"worst fp32 yardstick / tolerance: {worst:.3f} (must stay below 0.2)")
    print(lines[-1])
    if a.device:
        rep = {}
        check_bce(a.device, rep)
        check_ce(a.device, rep)
        check_head_criteria(a.device, rep)
        check_eval_scores(a.device, rep)
        check_masked_loss_edges(a.device)
        lines.append(f"B. criteria against float64 on the {where} (loss: of max(1, |ref|), bound {LOSS_TOL:.0e}; dlogits: of their maximum, bound "
                     f"{DLOGITS_TOL:.0e}; row_sum_x_B: bound {ROW_SUM_TOL:.0e}; probs: absolute, bound 1e-06)")
        lines += [f"{k:<40}" + "  ".join(f"{q} {v:.2e}" for q, v in e.items()) for k, e in rep.items()]
        rep = {}
        check_head_ties(a.device, rep)
        lines.append(f"C. head at ties and zeros on the {where} (arg and zero pattern exact; of max(floor, max |ref|), bound {LOSS_TOL:.0e})")
        lines += [f"{k:<56}" + "  ".join(f"{q} {v:.2e}" for q, v in e.items()) for k, e in rep.items()]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if worst < 0.2 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
