"""Checks of the occlusion maps on the device (eeg_gnn_ssl_amd/interpret.py, csrc/kernels_occlude.h): the expand kernel
(`ops.occlude_expand`) bit for bit against an ATen construction, the scores kernel (`ops.occlusion_scores`) against the float64
formula, whole maps against `oracle.classification_forward` in float64 on explicitly built variants that each run from step 0 (the
oracle knows nothing of prefix sharing), the launches a pass issues, `TrainStep.occlusion_maps`, the absence of side effects,
refusals and operator registration.  The same functions run on the GPU library and on the emulator build of the same kernel sources
(tests/test_occlusion.py).

Each check FAILS ON THE PARENT COMMIT: `ops.occlude_expand`, `ops.occlusion_scores`, `eeg_gnn_ssl_amd.interpret` and
`TrainStep.occlusion_maps` do not exist there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import TOL, kernels_run, load, make_args

N = 19
SCORE_ATOL = 1e-7                 # the float32 store of a value of magnitude <= 1 that was formed in double: half an ulp is 2^-25 = 3e-8


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _guarded(shape, device, dtype=torch.float32, fill=-5, sentinel=-77):
    """a buffer between one sentinel row in front and one behind -> (view, intact())"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), sentinel, dtype=dtype, device=device)
    buf[1:-1] = fill

    def intact():
        return bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    return buf[1:-1], intact


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _groups(kind, device):
    """None (G = N, group g = {g}) / "three": G = 3 -- nodes 0..8 (nine), nobody (empty), nodes 9, 12, 18 / "one": G = 1, nodes 3 and 4"""
    if kind is None:
        return None
    m = torch.zeros((3 if kind == "three" else 1), N, dtype=torch.int32)
    if kind == "three":
        m[0, :9] = 1
        m[2, [9, 12, 18]] = 1
    else:
        m[0, [3, 4]] = 1
    return m.to(device)


def _mask(groups):
    return torch.eye(N, dtype=torch.bool) if groups is None else groups.cpu().bool()


# ---- 1. the expand kernel alone -----------------------------------------------------------------------------------------------------------
def expand_by_aten(x, hext, mask, lens, t0, w, fill):
    """what `ops.occlude_expand` writes, made with ATen on the host: (x_var, h0_var, len_var)"""
    b, t, n, d = x.shape
    g = mask.shape[0]
    xv = x[:, t0:].unsqueeze(1).repeat(1, g, 1, 1, 1)                            # (B, G, T - t0, N, D)
    inside = min(w, t - t0)
    xv[:, :, :inside] = torch.where(mask[None, :, None, :, None], torch.tensor(fill, dtype=x.dtype), xv[:, :, :inside])
    xv = xv.reshape(b * g, t - t0, n, d).transpose(0, 1).contiguous()
    h0 = torch.stack([h[t0].repeat_interleave(g, dim=0) for h in hext], dim=0)
    full = torch.full((b,), t, dtype=torch.int64) if lens is None else lens
    return xv, h0, (full - t0).clamp(min=1).repeat_interleave(g)


# (B, T, D, H, L, groups, lengths, w, starts, fill).  The kernel's paths: rows of fewer pieces than a block has threads (D = 8: 38) and
# of more than two rounds of them (D = 200: 950; N*H = 19*64: 304 -- one full round and a ragged second); a step inside and behind the
# window; t0 = T - 1 (one step); a partial last window (T = 7, w = 2, t0 = 6); the empty group; G = 1; G split into stretches (few
# rows) and not split, with more rows than the capped grid holds (B = 64, T = 33: 2176 rows over at most 2048 blocks on the GPU, and
# every case here over the emulator's 32).
EXPAND_CASES = (
    (3, 7, 8, 16, 2, None, (7, 5, 1), 2, (0, 2, 6), 0.0),
    (3, 6, 100, 64, 2, "three", (6, 4, 1), 1, (0, 3, 5), 0.0),
    (2, 3, 200, 16, 3, "one", None, 1, (0, 2), -1.5),
    (5, 7, 8, 16, 4, "three", (9, 7, -3, 0, 2), 3, (0, 3, 6), 0.25),
    (64, 33, 4, 4, 1, "one", None, 5, (0, 30), 0.0),
)


def check_expand_kernel(device):
    """`ops.occlude_expand` on EXPAND_CASES: x_var, h0_var and len_var are bit-equal to `expand_by_aten` (a copy kernel: the tolerance
    is zero; the inputs carry a NaN, an infinity and a -0.0), and the sentinel rows around the three buffers stay intact."""
    from eeg_gnn_ssl_amd import ops
    gen = torch.Generator().manual_seed(11)
    for b, t, d, h, layers, kind, lens, w, starts, fill in EXPAND_CASES:
        x = torch.randn(b, t, N, d, generator=gen)
        x[0, 0, 0, 0], x[b - 1, t - 1, N - 1, d - 1], x[0, t // 2, 3, 1] = float("nan"), float("inf"), -0.0
        hext = [torch.randn(t + 1, b, N * h, generator=gen) for _ in range(layers)]
        lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int64)
        groups = _groups(kind, device)
        gmask = torch.eye(N, dtype=torch.int32, device=device) if groups is None else groups
        g = gmask.shape[0]
        xd, hd = x.to(device), [v.to(device) for v in hext]
        ld = None if lens_t is None else lens_t.to(device)
        for t0 in starts:
            tag = (b, t, d, h, layers, kind, t0)
            x_var, x_ok = _guarded((t - t0, b * g, N, d), device)
            h0_var, h_ok = _guarded((layers, b * g, N * h), device)
            len_var, l_ok = _guarded((b * g,), device, dtype=torch.int64)
            ops.occlude_expand(xd, hd, gmask, ld, t0, w, fill, x_var, h0_var, len_var)
            want_x, want_h, want_l = expand_by_aten(x, hext, _mask(groups), lens_t, t0, w, fill)
            assert x_ok() and h_ok() and l_ok(), tag
            assert torch.equal(_bits(x_var.cpu()), _bits(want_x)), tag
            assert torch.equal(_bits(h0_var.cpu()), _bits(want_h)), tag
            assert torch.equal(len_var.cpu(), want_l), tag
            if kind == "three" and t0 == 0:     # the case tells the groups apart: the empty one is the plain clip, the others are not
                plain = x[:, :w].transpose(0, 1)
                got = x_var.cpu()[:w].view(w, b, g, N, d)
                assert torch.equal(_bits(got[:, :, 1]), _bits(plain)) and not torch.equal(_bits(got[:, :, 0]), _bits(plain))


# ---- 2. the scores kernel alone -----------------------------------------------------------------------------------------------------------
def scores_by_formula(var_logits, base_logits, lens, target, t0):
    """float64 torch on the same float32 logits -> (maps slice (B, G), base_prob (B,), class followed (B,))"""
    b, c = base_logits.shape
    v, base = var_logits.double().view(b, -1, c), base_logits.double()
    if c == 1:
        cls = torch.zeros(b, dtype=torch.int64)
        pb, pv = torch.sigmoid(base[:, 0]), torch.sigmoid(v[:, :, 0])
    else:
        cls = base_logits.argmax(dim=1) if target is None else target.clamp(0, c - 1)
        pb = torch.softmax(base, dim=1).gather(1, cls[:, None])[:, 0]
        pv = torch.softmax(v, dim=2).gather(2, cls[:, None, None].expand(-1, v.shape[1], 1))[:, :, 0]
    out = pb[:, None] - pv
    if lens is not None:
        out = torch.where((lens > t0)[:, None], out, torch.zeros_like(out))
    return out, pb, cls


def check_scores_kernel(device):
    """`ops.occlusion_scores` on random logits (x3, one at +-30), B = 5, G = 3, Tw = 4, C = 1 and C = 4, lengths (9, 3, 1, 2, 4),
    windows k = 0..3 at t0 = 2k: the slice within 1e-7 of the float64 formula, exactly 0.0 where t0 >= len, the other slices
    untouched; base_prob and the class followed written by window 0 only; target=None takes the LOWEST index of a constructed tie
    (rows 1 and 3: two and four equal maxima); a target outside 0..C-1 is clamped (-3 -> 0, 9 -> 3); the guards stay intact."""
    from eeg_gnn_ssl_amd import ops
    gen = torch.Generator().manual_seed(7)
    b, g, tw = 5, 3, 4
    lens = torch.tensor([9, 3, 1, 2, 4], dtype=torch.int64)
    for c in (1, 4):
        base = torch.randn(b, c, generator=gen) * 3
        var = torch.randn(tw, b * g, c, generator=gen) * 3
        base[0, 0], var[0, 0, 0] = 30.0, -30.0
        targets = [None]
        if c == 4:
            base[1] = torch.tensor([0.5, 2.0, 2.0, -1.0])
            base[3] = torch.tensor([1.25, 1.25, 1.25, 1.25])
            targets = [None, torch.tensor([2, -3, 9, 0, 3], dtype=torch.int64)]
        for target in targets:
            for use_lens in (True, False):
                maps, m_ok = _guarded((b, tw, g), device)
                base_prob, p_ok = _guarded((b,), device)
                tgt_out, t_ok = _guarded((b,), device, dtype=torch.int64)
                ln = lens if use_lens else None
                for k in (3, 0, 1, 2):                                           # (any order: a window writes its own slice)
                    before = (base_prob.clone(), tgt_out.clone(), maps.clone())
                    ops.occlusion_scores(var[k].to(device), base.to(device), None if ln is None else ln.to(device),
                                         None if target is None else target.to(device), k, 2 * k, maps, base_prob,
                                         tgt_out if c > 1 else None)
                    want, pb, cls = scores_by_formula(var[k], base, ln, target, 2 * k)
                    got = maps.cpu()[:, k].double()
                    assert float((got - want).abs().max()) <= SCORE_ATOL, (c, k, float((got - want).abs().max()))
                    if ln is not None:
                        dead = ln <= 2 * k
                        assert bool((maps.cpu()[:, k][dead] == 0.0).all()) and (k == 0 or bool(dead.any()))
                    others = [j for j in range(tw) if j != k]
                    assert torch.equal(maps[:, others], before[2][:, others])
                    if k == 0:
                        assert float((base_prob.cpu().double() - pb).abs().max()) <= SCORE_ATOL
                        if c > 1:
                            assert torch.equal(tgt_out.cpu(), cls), (tgt_out, cls)
                            if target is None:
                                assert cls[1].item() == 1 and cls[3].item() == 0
                            else:
                                assert tgt_out.cpu().tolist() == [2, 0, 3, 0, 3]
                        else:
                            assert bool((tgt_out == -5).all())
                    else:
                        assert torch.equal(base_prob, before[0]) and torch.equal(tgt_out, before[1])
                assert m_ok() and p_ok() and t_ok(), (c, use_lens)
                assert bool((maps.cpu().abs() <= 1.0).all())


# ---- 3. / 4. whole maps against the oracle ------------------------------------------------------------------------------------------------
# name -> (filter, classes, D, T, w, groups, target, clips_per_pass).  B = 3 with lengths (T, T - 2, 1): the last clip makes every window
# behind the first a zero row; T = 6 with w = 1 and T = 7 with w = 2 (a partial last window).  "lap": laplacian K = 2 on the 2-D
# distance graph (the spectral form at 64 units); "drw": dual_random_walk K = 2 with per-clip batched supports (the correlation graphs
# of the clips) and 4 classes (the general path).
MAP_CASES = {
    "lap_d8_t6_w1": ("laplacian", 1, 8, 6, 1, None, None, 16),
    "lap_d100_t7_w2_chunks": ("laplacian", 1, 100, 7, 2, None, None, 2),
    "drw_d100_t6_w1_argmax": ("dual_random_walk", 4, 100, 6, 1, None, None, 16),
    "drw_d8_t7_w2_groups_target_chunks": ("dual_random_walk", 4, 8, 7, 2, "three", (3, 0, 2), 2),
}
B = 3


@functools.lru_cache(maxsize=None)
def _map_case(name, units, adj_key):
    """the inputs of a case and the oracle's answer, computed ONCE per (case, units) and shared by the checks (never modified):
    float64 `classification_forward` on the unoccluded clips and on every variant, built explicitly and run from step 0"""
    filt, classes, d, t, w, gkind, target, _ = MAP_CASES[name]
    adj3d = np.frombuffer(adj_key[0], dtype=adj_key[1]).reshape(adj_key[2])
    cfg = orc.DCRNNConfig(filter_type=filt, input_dim=d, num_classes=classes, rnn_units=units)
    params = orc.init_params(cfg, "classification", seed=1)
    x = torch.randn(B, t, N, d, generator=torch.Generator().manual_seed(5))
    lens = torch.tensor([t, t - 2, 1], dtype=torch.int64)
    if filt == "laplacian":
        supports = orc.compute_supports(adj3d, "laplacian")
    else:                                   # one graph per clip: the top-3 correlation graphs of the unpadded clips, made by the oracle
        mats = [orc.compute_supports(orc.correlation_adjacency(x[i, :int(lens[i])].numpy(), top_k=3), filt) for i in range(B)]
        supports = [torch.stack([m[j] for m in mats], dim=0) for j in range(2)]
    mask = _mask(_groups(gkind, "cpu"))
    g, tw = mask.shape[0], -(-t // w)
    x64 = x.double()
    variants = x64[:, None, None].repeat(1, tw, g, 1, 1, 1)                      # (B, Tw, G, T, N, D)
    for k in range(tw):
        for gi in range(g):
            variants[:, k, gi, k * w:min((k + 1) * w, t), mask[gi]] = 0.0
    rep = lambda s: s.double() if s.dim() == 2 else torch.cat([s, s.repeat_interleave(tw * g, dim=0)], dim=0).double()     # noqa: E731
    p64 = {k_: v.double() for k_, v in params.items()}
    logits = orc.classification_forward(p64, cfg, torch.cat([x64, variants.reshape(B * tw * g, t, N, d)], dim=0),
                                        torch.cat([lens, lens.repeat_interleave(tw * g)]), [rep(s) for s in supports])
    base, var = logits[:B], logits[B:].view(B, tw, g, classes)
    tgt = None if target is None else torch.tensor(target, dtype=torch.int64)
    if classes == 1:
        cls, pb, pv = None, torch.sigmoid(base[:, 0]), torch.sigmoid(var[..., 0])
    else:
        cls = base.argmax(dim=1) if tgt is None else tgt
        pb = torch.softmax(base, dim=1).gather(1, cls[:, None])[:, 0]
        pv = torch.softmax(var, dim=3).gather(3, cls[:, None, None, None].expand(-1, tw, g, 1))[..., 0]
    live = (torch.arange(tw) * w)[None, :] < lens[:, None]                       # (B, Tw): window start < len_b
    maps = torch.where(live[:, :, None], pb[:, None, None] - pv, torch.zeros_like(pv))
    return dict(cfg=cfg, params=params, x=x, lens=lens, supports=supports, groups=gkind, target=tgt, w=w, base=base, var=var, cls=cls,
                pb=pb, maps=maps, live=live, scale=float(logits.abs().max()))


def map_case(name, units, adj3d):
    a = np.ascontiguousarray(adj3d)
    return _map_case(name, units, (a.tobytes(), a.dtype.str, a.shape))


def _model(case, device):
    from eeg_gnn_ssl_amd import DCRNNModel_classification
    model = DCRNNModel_classification(make_args(case["cfg"]), case["cfg"].num_classes, device=device)
    load(model, case["params"], device)
    return model


def _run(case, model, device, **kw):
    from eeg_gnn_ssl_amd import occlusion_maps
    args = dict(time_window=case["w"], node_groups=_groups(case["groups"], device),
                target=None if case["target"] is None else case["target"].to(device), return_logits=True)
    args.update(kw)
    return occlusion_maps(model, case["x"].to(device), case["lens"].to(device), [s.to(device) for s in case["supports"]], **args)


def _assert_maps(res, case, what):
    """variant logits at TOL relative to the oracle's largest |logit|; maps at the ABSOLUTE tolerance TOL * max|logit| -- derived: an
    entry is the difference of two probabilities, the sigmoid's slope is at most 1/4 and the L1 norm of a softmax probability's
    gradient at most 1/2, so logit errors of TOL * max|logit| move it by less than that; dead entries are exactly 0.0"""
    scale = case["scale"]
    tol = TOL * scale
    e_base = float((res.base_logits.cpu().double() - case["base"]).abs().max())
    e_var = float((res.variant_logits.cpu().double() - case["var"]).abs().max())
    e_map = float((res.maps.cpu().double() - case["maps"]).abs().max())
    e_pb = float((res.base_prob.cpu().double() - case["pb"]).abs().max())
    print(f"{what}: max|logit| {scale:.3f}, errors: baseline logits {e_base:.2e}, variant logits {e_var:.2e}, maps {e_map:.2e}, "
          f"base_prob {e_pb:.2e} (tolerance {tol:.2e}); largest |map| {float(case['maps'].abs().max()):.2e}")
    assert e_base <= tol and e_var <= tol, (what, e_base, e_var, tol)
    assert e_map <= tol and e_pb <= tol, (what, e_map, e_pb, tol)
    dead = ~case["live"][:, :, None].expand_as(case["maps"])
    assert bool((res.maps.cpu()[dead] == 0.0).all()), what
    if case["cls"] is None:
        assert res.target is None
    else:
        assert torch.equal(res.target.cpu(), case["cls"]), (what, res.target, case["cls"])


def check_maps(device, adj3d, name, units):
    """`occlusion_maps(..., return_logits=True)` on one of MAP_CASES against the oracle (`_assert_maps`).  Before that, on the ORACLE's
    values, the condition that keeps the comparison from passing on noise: its largest |map| is at least 1e-3 and at least 80 % of the
    live entries (window start < len_b) are at least 1e-4 -- the tolerance is about 100 times below the median entry.  (The case with
    an EMPTY group: a third of its entries are 0 by definition, asserted to be exactly that, and the condition is taken over the live
    entries of the two other groups.)"""
    from eeg_gnn_ssl_amd import ops
    case = map_case(name, units, adj3d)
    live = case["live"][:, :, None].expand_as(case["maps"])
    mags = case["maps"][live].abs()
    if case["groups"] == "three":           # (the empty group's entries are exactly 0 by construction: they are not what the condition is about)
        keep = torch.ones_like(case["maps"], dtype=torch.bool)
        keep[:, :, 1] = False
        assert bool((case["maps"][:, :, 1] == 0.0).all())
        mags = case["maps"][live & keep].abs()
    assert float(mags.max()) >= 1e-3, float(mags.max())
    assert float((mags >= 1e-4).double().mean()) >= 0.8, float((mags >= 1e-4).double().mean())
    assert bool((case["maps"][~live] == 0.0).all()) and int((~live).sum()) > 0
    model = _model(case, device)
    before = ops.spectral_layer_calls
    res = _run(case, model, device, clips_per_pass=MAP_CASES[name][7])
    if case["cfg"].filter_type == "laplacian" and units == 64:
        assert ops.spectral_layer_calls > before, "the shared 2-D graph takes the spectral form, for the variants as for the baseline"
    if case["cfg"].filter_type == "dual_random_walk":
        assert ops.spectral_layer_calls == before, "per-clip supports take the general path"
    g = case["maps"].shape[2]
    assert res.maps.shape == case["maps"].shape and res.variant_logits.shape == case["var"].shape and res.maps.dtype == torch.float32
    assert res.base_prob.shape == (B,) and res.base_logits.shape == (B, case["cfg"].num_classes) and g in (3, N)
    _assert_maps(res, case, f"{name} ({units} units)")
    assert model.training


# ---- 5. prefix sharing really happens -------------------------------------------------------------------------------------------------------
def check_prefix_sharing(device, adj3d, units):
    """On "lap_d8_t6_w1" and "drw_d8_t7_w2_groups_target_chunks" with the event recorder on: one pass over one chunk issues exactly Tw
    launches under each of `occlude_expand` and `occlusion_scores`.  A variant's logits out of the prefix-shared pass equal, within
    tolerance, what the same function computes with time_window = T -- a single window that starts at step 0 and so needs no
    baseline state: on the explicitly occluded clip with one EMPTY group (its baseline and its one variant are that clip from step
    0), and on the plain clip against the oracle's one-window map.  clips_per_pass = B and clips_per_pass = 2 agree within the
    map tolerance."""
    from eeg_gnn_ssl_amd import occlusion_maps
    for name in ("lap_d8_t6_w1", "drw_d8_t7_w2_groups_target_chunks"):
        case = map_case(name, units, adj3d)
        model = _model(case, device)
        tw, g = case["maps"].shape[1:]
        t, w = case["x"].shape[1], case["w"]
        out = {}
        ran = kernels_run(lambda: out.update(res=_run(case, model, device, clips_per_pass=B)))
        res = out["res"]
        assert sum(ran.get("occlude_expand", {}).values()) == tw and sum(ran.get("occlusion_scores", {}).values()) == tw, ran
        tol = TOL * case["scale"]
        _assert_maps(res, case, f"{name} one chunk")
        # (a) from step 0, no baseline state: the occluded clip itself through a single window with an empty group
        mask = _mask(_groups(case["groups"], "cpu"))
        empty = torch.zeros(1, N, dtype=torch.int32, device=device)
        sup = [s.to(device) for s in case["supports"]]
        for k, gi in ((0, 0), (tw // 2, g - 1), (tw - 1, 0)):
            xo = case["x"].clone()
            xo[:, k * w:min((k + 1) * w, t), mask[gi]] = 0.0
            one = occlusion_maps(model, xo.to(device), case["lens"].to(device), sup, time_window=t, node_groups=empty,
                                 target=None if case["target"] is None else case["target"].to(device), return_logits=True)
            assert one.maps.shape == (B, 1, 1) and bool((one.maps == 0.0).all())          # an empty group occludes nothing: p - p
            assert torch.equal(one.variant_logits[:, 0, 0], one.base_logits)
            err = float((one.base_logits.cpu().double() - res.variant_logits.cpu().double()[:, k, gi]).abs().max())
            assert err <= tol, (name, k, gi, err, tol)
        # (b) the plain clip, one window over all steps, against variants the oracle runs from step 0
        whole = occlusion_maps(model, case["x"].to(device), case["lens"].to(device), sup, time_window=t,
                               node_groups=_groups(case["groups"], device), target=None if case["target"] is None else case["target"].to(device),
                               return_logits=True)
        x64 = case["x"].double()[:, None].repeat(1, g, 1, 1, 1)
        for gi in range(g):
            x64[:, gi, :, mask[gi]] = 0.0
        rep = lambda s: s.double() if s.dim() == 2 else s.repeat_interleave(g, dim=0).double()     # noqa: E731
        want = orc.classification_forward({k_: v.double() for k_, v in case["params"].items()}, case["cfg"], x64.reshape(B * g, t, N, -1),
                                          case["lens"].repeat_interleave(g), [rep(s) for s in case["supports"]]).view(B, g, -1)
        err = float((whole.variant_logits.cpu().double()[:, 0] - want).abs().max())
        assert whole.maps.shape == (B, 1, g) and err <= tol, (name, err, tol)
        # (c) chunks
        two = _run(case, model, device, clips_per_pass=2)
        assert float((two.maps - res.maps).abs().max()) <= tol and float((two.variant_logits - res.variant_logits).abs().max()) <= tol
        assert torch.equal(two.target, res.target) if res.target is not None else two.target is None


# ---- 6. TrainStep.occlusion_maps, no side effects --------------------------------------------------------------------------------------------
W = 8


def _step_case(kind, device, units):
    """-> (model, TrainStep keywords, task, raw x (B, N, T*W), lengths): "raw_fft" (raw signals -> log|FFT| -> z-score, detection, variable
    lengths with padding_val: the graph of the unpadded clip) / "time_domain" (use_fft=False: windows, 4 classes, full lengths)"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification
    t = 6
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, N, t * W, generator=g).to(device)
    if kind == "raw_fft":
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W // 2, num_classes=1, rnn_units=units)
        kw, task, lens = dict(raw_window=W, raw_mean=0.3, raw_std=1.7, padding_val=0.0), "detection", torch.tensor([t, t - 2, 1]).to(device)
    else:
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W, num_classes=4, rnn_units=units)
        kw, task, lens = dict(raw_window=W, raw_mean=0.3, raw_std=1.7, use_fft=False), "classification", None
    model = DCRNNModel_classification(make_args(cfg), cfg.num_classes, device=device)
    load(model, orc.init_params(cfg, "classification", seed=6), device)
    return model, kw, task, x, lens


def check_train_step(device, kind, units):
    """`TrainStep.occlusion_maps(raw x, lengths, supports=None)` on a raw pool and on a time-domain pool equals, bit for bit,
    `occlusion_maps` on the features and supports `_data_chain` returns (the correlation graph of the unpadded clip, built once);
    the maps are not all zero and have the shape (B, ceil(T / 2), G)"""
    from eeg_gnn_ssl_amd import occlusion_maps
    from eeg_gnn_ssl_amd.train_step import TrainStep
    model, kw, task, x, lens = _step_case(kind, device, units)
    st = TrainStep(model, task=task, **kw)
    groups = _groups("three", device)
    got = st.occlusion_maps(x, lens, None, time_window=2, node_groups=groups, return_logits=True)
    with torch.no_grad():
        feats, _, sup = st._data_chain(x, None, lens, None)
    assert feats.shape == (B, 6, N, W // 2 if kind == "raw_fft" else W) and all(s.shape == (B, N, N) for s in sup)
    want = occlusion_maps(model, feats, lens, sup, time_window=2, node_groups=groups, return_logits=True)
    for u, v in zip(got, want):
        assert (u is None and v is None) or torch.equal(u, v), kind
    assert got.maps.shape == (B, 3, 3) and float(got.maps.abs().max()) > 0 and bool((got.maps[:, :, 1] == 0.0).all())
    if lens is not None:
        assert bool((got.maps[2, 1:] == 0.0).all()) and float(got.maps[2, 0].abs().max()) > 0
    assert (got.target is None) == (task == "detection") and model.training


def check_no_side_effects(device, adj3d, units=16):
    """a `TrainStep(data_augment=True)` over a dropout model in train mode, one training step taken (Adam moments non-zero): after
    `TrainStep.occlusion_maps` the parameters, the optimiser state, step_count / samples_seen and their device mirrors, the two Philox
    states, the sampler slot, the learning rate and model.training are bit-equal to what they were, and the maps equal those of a twin
    without dropout or augmentation over the same parameters"""
    import copy
    from eeg_gnn_ssl_amd import DCRNNModel_classification, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    d, t = 8, 6
    cfg = orc.DCRNNConfig(filter_type="laplacian", input_dim=d, num_classes=1, rnn_units=units)
    args = copy.copy(make_args(cfg))
    args.dropout = 0.5
    noisy = DCRNNModel_classification(args, 1, device=device)
    load(noisy, orc.init_params(cfg, "classification", seed=6), device)
    noisy.train()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, t, N, d, generator=g).to(device)
    y = torch.tensor([1.0, 0.0, 1.0]).to(device)
    lens = torch.tensor([t, t - 2, 1]).to(device)
    supports = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")]
    torch.manual_seed(3)
    st = TrainStep(noisy, task="detection", data_augment=True, feature_std=1.7)
    st.step(x, y, lens, supports)

    def state():
        return (noisy.training, st.step_count, st.samples_seen, st.step_dev.clone(), st.samples_seen_dev.clone(), st.fp.flat.detach().clone(),
                st.fp.flat_grad.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(), st._augment_rng.clone(), noisy._dropout_rng.clone(),
                id(st.sampler), st.lr, torch.is_grad_enabled())

    before = state()
    assert bool(st.exp_avg.abs().sum() > 0) and noisy.training and st.step_count == 1
    res = st.occlusion_maps(x, lens, supports, time_window=2)
    for u, v in zip(before, state()):
        assert torch.equal(u, v) if torch.is_tensor(u) else u == v
    plain = DCRNNModel_classification(make_args(cfg), 1, device=device)
    plain.load_state_dict(noisy.state_dict())
    plain.to(device).eval()
    res2 = TrainStep(plain, task="detection").occlusion_maps(x, lens, supports, time_window=2)
    assert torch.equal(res.maps, res2.maps) and torch.equal(res.base_prob, res2.base_prob) and not plain.training
    assert float(res.maps.abs().max()) > 0 and res.variant_logits is None


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d):
    """every refusal of `occlusion_maps` / `TrainStep.occlusion_maps` is a ValueError raised BEFORE any launch (the event recorder sees
    none): rank and dtype of x, D % 4, a misaligned view, node_groups of another shape / dtype / device, time_window < 1, G outside
    1..64, more than 4 layers, a target for a one-output head, a head that does not fit the task, task="ssl"; the operators and the C
    entry points refuse what the host layer cannot produce"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, _lib, occlusion_maps, ops, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    d, t = 8, 4
    cfg = orc.DCRNNConfig(filter_type="laplacian", input_dim=d, num_classes=1, rnn_units=16)
    model = DCRNNModel_classification(make_args(cfg), 1, device=device).to(device)
    sup = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")]
    x, lens = z(B, t, N, d), torch.full((B,), t, dtype=torch.int64, device=device)
    deep = DCRNNModel_classification(make_args(orc.DCRNNConfig(filter_type="laplacian", input_dim=d, num_rnn_layers=5, rnn_units=16)), 1).to(device)
    four = DCRNNModel_classification(make_args(orc.DCRNNConfig(filter_type="laplacian", input_dim=d, num_classes=4, rnn_units=16)), 4).to(device)
    ssl = DCRNNModel_nextTimePred(make_args(orc.DCRNNConfig(filter_type="laplacian", input_dim=d, output_dim=d, rnn_units=16)), device=device).to(device)
    odd = z(B * t * N * d + 1)[1:].view(B, t, N, d)             # contiguous, 4 bytes off a 16-byte boundary
    other = "meta" if device == "cpu" else "cpu"

    def refused():
        for bad, pattern, kw in (
                (z(B, t, N * d), r"x must be \(B, T, N, D\) float32", {}),
                (x.double(), r"x must be \(B, T, N, D\) float32", {}),
                (z(B, t, N, 6), r"D=6.*multiple of 4", {}),
                (z(B, t, N + 1, d), r"x has 20 nodes, the model 19", {}),
                (odd, r"not 16-byte aligned", {}),
                (x, r"node_groups must be a \(G, 19\) int32", dict(node_groups=z(3, N + 1, dtype=torch.int32))),
                (x, r"node_groups must be a \(G, 19\) int32", dict(node_groups=z(3, N))),
                (x, r"node_groups must be a \(G, 19\) int32", dict(node_groups=torch.zeros(3, N, dtype=torch.int32, device=other))),
                (x, r"G=65 groups", dict(node_groups=z(65, N, dtype=torch.int32))),
                (x, r"G=0 groups", dict(node_groups=z(0, N, dtype=torch.int32))),
                (x, r"time_window=0", dict(time_window=0)),
                (x, r"time_window=1.5", dict(time_window=1.5)),
                (x, r"clips_per_pass=0", dict(clips_per_pass=0)),
                (x, r"target names the class", dict(target=lens)),
                (x, r"seq_lengths must be an int64", dict(seq_lengths=lens.int()))):
            kw = dict(kw)
            ln = kw.pop("seq_lengths", lens)
            with pytest.raises(ValueError, match=pattern):
                occlusion_maps(model, bad, ln, sup, **kw)
        with pytest.raises(ValueError, match=r"5 layers, one pass takes at most 4"):
            occlusion_maps(deep, x, lens, sup)
        with pytest.raises(ValueError, match=r"target must be an int64 tensor of shape \(3,\)"):
            occlusion_maps(four, x, lens, sup, target=torch.zeros(B + 1, dtype=torch.int64, device=device))
        with pytest.raises(ValueError, match=r"task='ssl'.*ssl_evaluator"):
            TrainStep(ssl, task="ssl").occlusion_maps(x, lens, sup)
        with pytest.raises(ValueError, match=r"task='classification'\): the model's head has 1 outputs"):
            TrainStep(model, task="classification").occlusion_maps(x, lens, sup)
        with pytest.raises(ValueError, match=r"task='detection'\): the model's head has 4 outputs"):
            TrainStep(four, task="detection").occlusion_maps(x, lens, sup)
        with pytest.raises(ValueError, match=r"time_window=-1"):
            TrainStep(model, task="detection", raw_window=W).occlusion_maps(z(B, N, t * W), lens, None, time_window=-1)

    ran = kernels_run(refused)
    assert ran == {}, f"a refusal came behind a launch: {ran}"
    # the operators
    eye = torch.eye(N, dtype=torch.int32, device=device)
    hext = [z(t + 1, B, N * 16), z(t + 1, B, N * 16)]
    xv, hv, lv = z(t, B * N, N, d), z(2, B * N, N * 16), z(B * N, dtype=torch.int64)
    for args, pattern in (
            ((x, hext, eye, lens, t, 1, 0.0, xv, hv, lv), r"a window of w=1 steps at t0=4 of T=4"),
            ((x, hext, eye, lens, 0, 0, 0.0, xv, hv, lv), r"a window of w=0 steps"),
            ((x, hext, eye, lens, 1, 1, 0.0, xv, hv, lv), r"x_var must be .*shape \(3, 57, 19, 8\)"),
            ((x, hext, eye.long(), lens, 0, 1, 0.0, xv, hv, lv), r"groups must be a contiguous torch.int32"),
            ((x, hext * 3, eye, lens, 0, 1, 0.0, xv, hv, lv), r"6 layers \(1..4"),
            ((x, hext, eye, lens.int(), 0, 1, 0.0, xv, hv, lv), r"lengths must be a contiguous torch.int64"),
            ((x, [hext[0], z(t + 1, B, N * 8)], eye, lens, 0, 1, 0.0, xv, hv, lv), r"hext\[1\] must be .*shape \(5, 3, 304\)"),
            ((x, hext, eye, lens, 0, 1, 0.0, xv, hv[:, :-1], lv), r"h0_var must be a contiguous"),
            ((odd, hext, eye, lens, 0, 1, 0.0, xv, hv, lv), r"x is not 16-byte aligned")):
        with pytest.raises(RuntimeError, match=pattern):
            ops.occlude_expand(*args)
    maps, bp, lg, bl = z(B, 2, N), z(B), z(B * N, 4), z(B, 4)
    for args, pattern in (
            ((lg, bl, lens, None, 2, 0, maps, bp), r"window k=2 of Tw=2"),
            ((lg[:-1], bl, lens, None, 0, 0, maps, bp), r"var_logits must be .*shape \(57, 4\)"),
            ((lg, bl, lens, lens.int(), 0, 0, maps, bp), r"target must be a contiguous torch.int64"),
            ((lg, z(B + 1, 4), lens, None, 0, 0, maps, bp), r"base_logits must be \(3, C\)"),
            ((lg, bl, lens, None, 0, 0, maps, z(B + 1)), r"base_prob must be .*shape \(3,\)")):
        with pytest.raises(RuntimeError, match=pattern):
            ops.occlusion_scores(*args)
    # C ABI
    lib = _lib.get_lib()
    p = lambda v: ctypes.c_void_p(v.data_ptr())     # noqa: E731
    tab = (ctypes.c_void_p * 2)(*[h.data_ptr() for h in hext])

    def no(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    fl = ctypes.c_float(0.0)
    no(lib.query("eeg_dcrnn_occlude_expand", None, tab, 2, p(eye), p(lens), B, t, N, d, 16, N, 0, 1, fl, p(xv), p(hv), p(lv), None), "null x")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 2, p(eye), p(lens), B, t, N, d, 16, N, 0, 1, fl, p(xv), None, p(lv), None), "null x_var / h0_var")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 5, p(eye), p(lens), B, t, N, d, 16, N, 0, 1, fl, p(xv), p(hv), p(lv), None), "5 layers")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 2, p(eye), p(lens), B, t, N, d, 16, 65, 0, 1, fl, p(xv), p(hv), p(lv), None), "G=65")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 2, p(eye), p(lens), B, t, N, 6, 16, N, 0, 1, fl, p(xv), p(hv), p(lv), None), "D=6")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 2, p(eye), p(lens), B, t, N, d, 16, N, t, 1, fl, p(xv), p(hv), p(lv), None), "t0=4 of T=4")
    no(lib.query("eeg_dcrnn_occlude_expand", p(x), tab, 2, p(eye), p(lens), B, t, 33, d, 16, N, 0, 1, fl, p(xv), p(hv), p(lv), None), "num_nodes=33")
    no(lib.query("eeg_dcrnn_occlude_expand", p(odd), tab, 2, p(eye), p(lens), B, t, N, d, 16, N, 0, 1, fl, p(xv), p(hv), p(lv), None), "16-byte aligned")
    no(lib.query("eeg_dcrnn_occlusion_scores", None, p(bl), p(lens), None, B, N, 4, 2, 0, 0, p(maps), p(bp), None, None), "null variant")
    no(lib.query("eeg_dcrnn_occlusion_scores", p(lg), p(bl), p(lens), None, B, N, 4, 2, 2, 0, p(maps), p(bp), None, None), "k=2 of Tw=2")
    no(lib.query("eeg_dcrnn_occlusion_scores", p(lg), p(bl), p(lens), None, B, 65, 4, 2, 0, 0, p(maps), p(bp), None, None), "G=65")
    no(lib.query("eeg_dcrnn_occlusion_scores", p(lg), p(bl), p(lens), None, B, N, 0, 2, 0, 0, p(maps), p(bp), None, None), "C=0")
    for v in (xv, hv, lv, maps, bp):                            # no refused call wrote anything
        assert bool((v == 0).all())


# ---- 8. operator registration ----------------------------------------------------------------------------------------------------------------
def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on both operators"""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    dv = lambda v: v.to(device)     # noqa: E731
    b, t, d, h, gr = 2, 3, 8, 16, 3
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    x = dv(torch.randn(b, t, N, d, generator=g))
    hext = [dv(torch.randn(t + 1, b, N * h, generator=g)) for _ in range(2)]
    lens = dv(torch.tensor([3, 1], dtype=torch.int64))
    samples = [
        (E.occlude_expand.default, (x, hext, _groups("three", device), lens, 1, 1, 0.0, z(t - 1, b * gr, N, d), z(2, b * gr, N * h),
                                    z(b * gr, dtype=torch.int64))),
        (E.occlude_expand.default, (x, hext[:1], _groups("one", device), None, 0, 2, 0.5, z(t, b, N, d), z(1, b, N * h), z(b, dtype=torch.int64))),
        (E.occlusion_scores.default, (dv(torch.randn(b * gr, 1, generator=g)), dv(torch.randn(b, 1, generator=g)), lens, None, 0, 0, z(b, 2, gr), z(b), None)),
        (E.occlusion_scores.default, (dv(torch.randn(b * gr, 4, generator=g)), dv(torch.randn(b, 4, generator=g)), None, dv(torch.tensor([1, 7])), 1, 2,
                                      z(b, 2, gr), z(b), z(b, dtype=torch.int64))),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
