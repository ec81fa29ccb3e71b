"""Occlusion maps on the device: the quantitative interpretability method of the paper behind the model.

For every clip one group of channels is overwritten with a fill value over one window of steps, and the map records how far the
predicted probability drops.  `occlusion_maps` shares the prefix of every variant with the unoccluded clip: an occlusion that starts
at step t0 leaves every state before t0 untouched, so the B*G variants of a window start from the baseline's states at t0 (every
layer returns them: `hext`) and run only T - t0 steps -- over all windows (T+1)/2T of the recurrent work of running every variant
from step 0.  The variant batches are built on the device (`ops.occlude_expand`, one launch per window) and scored there
(`ops.occlusion_scores`); the existing layer operators do the rest.

Semantics
    x (B, T, N, D) float32      the model's input (standardised features or windows)
    seq_lengths (B,) int64      or None: every clip has T steps
    supports                    as `DCRNNModel_classification.forward` takes them: 2-D shared, or batched per clip
    time windows                time_window = w >= 1, Tw = ceil(T / w); window k covers the steps [k*w, min((k+1)*w, T))
    node groups                 None: G = N and group g = {g}; else a (G, N) 0/1 mask, int32 on the device, 1 <= G <= 64 (hemispheres,
                                regions, any set of channels); an empty group is legal and occludes nothing
    variant (b, k, g)           clip b with x[b, t, n, :] = fill for t in window k and n in group g; fill = 0.0 is the feature mean
                                behind the z-score
    graph                       held FIXED: a variant runs on the supports of the unoccluded clip (with correlation graphs: built once,
                                from the clip as given) -- rebuilding it would mix two effects and cost a Gram per variant
    map value                   maps[b, k, g] = p_b - p_{b,k,g}; one output: p = sigmoid(logit); C classes: p = softmax(logits)[target_b],
                                target an int64 (B,) device tensor -- a class outside 0..C-1 is CLAMPED in the kernel -- or None: the
                                arg-max of the baseline logits, lowest index on ties.  A window that starts at or behind the clip's
                                end (k*w >= len_b) gets exactly 0.0.  The relative map maps / base_prob is left to the caller.
    mode                        eval: dropout off, no gradients, nothing saved for a backward; the model's mode is put back
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops


class OcclusionResult(NamedTuple):
    """maps (B, Tw, G), base_prob (B,), base_logits (B, C), target (B,) int64 (None for a one-output head), variant_logits
    (B, Tw, G, C) or None.  variant_logits of a window that starts at or behind the clip's end are the baseline's logits (the
    occlusion lies behind everything the model reads)."""
    maps: torch.Tensor
    base_prob: torch.Tensor
    base_logits: torch.Tensor
    target: Optional[torch.Tensor]
    variant_logits: Optional[torch.Tensor]


def _refuse(msg):
    raise ValueError("occlusion_maps: " + msg)


def _check_options(model, n, device, time_window, node_groups, clips_per_pass):
    """the refusals that do not need the features -> (layers, G)"""
    layers = len(model.encoder.encoding_cells)
    if not 1 <= layers <= ops.OCCLUDE_MAX_LAYERS:
        _refuse(f"the encoder has {layers} layers, one pass takes at most {ops.OCCLUDE_MAX_LAYERS} (ops.OCCLUDE_MAX_LAYERS)")
    if isinstance(time_window, bool) or not isinstance(time_window, int) or time_window < 1:
        _refuse(f"time_window={time_window!r} must be an integer >= 1")
    if isinstance(clips_per_pass, bool) or not isinstance(clips_per_pass, int) or clips_per_pass < 1:
        _refuse(f"clips_per_pass={clips_per_pass!r} must be an integer >= 1")
    if node_groups is None:
        g = n
    else:
        if not torch.is_tensor(node_groups) or node_groups.dim() != 2 or node_groups.shape[1] != n or node_groups.dtype != torch.int32 \
                or node_groups.device != device:
            got = f"{node_groups.dtype} {tuple(node_groups.shape)} on {node_groups.device}" if torch.is_tensor(node_groups) else type(node_groups).__name__
            _refuse(f"node_groups must be a (G, {n}) int32 0/1 mask on {device}, got {got}")
        g = int(node_groups.shape[0])
    if not 1 <= g <= ops.OCCLUDE_MAX_GROUPS:
        _refuse(f"G={g} groups, one pass takes 1..{ops.OCCLUDE_MAX_GROUPS} (ops.OCCLUDE_MAX_GROUPS)")
    return layers, g


def _check_inputs(model, x, seq_lengths, supports, time_window, node_groups, target, clips_per_pass):
    """every refusal, before any launch -> (x contiguous, groups (G, N) int32 or None, layers, classes)"""
    if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32:
        _refuse(f"x must be (B, T, N, D) float32, got {str(x.dtype) + ' ' + str(tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__}")
    b, t, n, d = (int(v) for v in x.shape)
    if b < 1 or t < 1:
        _refuse(f"x holds B={b} clips of T={t} steps")
    if n != model.num_nodes:
        _refuse(f"x has {n} nodes, the model {model.num_nodes}")
    if d < 4 or d % 4 != 0:
        _refuse(f"D={d}: the rows move in 16-byte pieces, D must be a positive multiple of 4")
    if (n * model.rnn_units) % 4 != 0:
        _refuse(f"num_nodes * rnn_units = {n * model.rnn_units} must be a multiple of 4")
    layers, g = _check_options(model, n, x.device, time_window, node_groups, clips_per_pass)
    classes = int(model.fc.weight.shape[0])
    if classes != int(getattr(model, "num_classes", classes)):
        _refuse(f"the head has {classes} outputs, the model num_classes={model.num_classes}")
    for name, v in (("seq_lengths", seq_lengths), ("target", target)):
        if v is not None and (not torch.is_tensor(v) or v.dtype != torch.int64 or tuple(v.shape) != (b,) or v.device != x.device):
            got = f"{v.dtype} {tuple(v.shape)} on {v.device}" if torch.is_tensor(v) else type(v).__name__
            _refuse(f"{name} must be an int64 tensor of shape ({b},) on {x.device} (read on the device), got {got}")
    if target is not None and classes == 1:
        _refuse("target names the class a map follows; this head has one output (detection): pass target=None")
    if not isinstance(supports, (list, tuple)) or not supports or not all(torch.is_tensor(s) and s.dim() in (2, 3) for s in supports):
        _refuse("supports must be a list of (N, N) tensors (shared) or (B, N, N) tensors (one graph per clip)")
    for s in supports:
        if s.dim() == 3 and s.shape[0] != b:
            _refuse(f"batched supports hold {s.shape[0]} graphs for {b} clips")
    x = x.contiguous()
    if x.data_ptr() % 16 != 0:
        _refuse("x is not 16-byte aligned (a view with an odd element offset): pass a tensor of its own")
    return x, node_groups, layers, classes


def _baseline(model, x, supports, lengths):
    """the unoccluded pass through the encoder cells the way `DCRNNEncoder.run` makes it, keeping every layer's state sequence
    -> ([hext_l (T+1, B, N*H)], top state at len - 1 (B, N*H))"""
    enc = model.encoder
    b, t_len = x.shape[0], x.shape[1]
    enc.encoding_cells[0]._check_supports(supports)
    p, p_batched = ops.hop_polys(supports, enc.max_diffusion_step, b)
    basis = ops.shared_spectral_basis(supports, enc.max_diffusion_step)
    packs = ops.pack_encoder_cells(enc.encoding_cells, basis, enc.num_nodes)
    cur, x_off, planes = x.transpose(0, 1), 0, None
    hexts, out = [], None
    for layer, cell in enumerate(enc.encoding_cells):
        is_top = layer == enc.num_rnn_layers - 1
        out = cell.run_sequence(cur, None, p, p_batched, lengths if is_top else None, x_off, planes, want_hsel=is_top, basis=basis,
                                pack=None if packs is None else packs[0][layer], spack=None if packs is None else packs[1][layer])
        hexts.append(out.hext)
        cur, x_off, planes = out.hext.view(t_len + 1, b, enc.num_nodes, enc.hid_dim), 1, out.hpl
    return hexts, out.hsel


@torch.no_grad()
def occlusion_maps(model, x, seq_lengths, supports, *, time_window: int = 1, node_groups=None, fill: float = 0.0, target=None,
                   clips_per_pass: int = 16, return_logits: bool = False) -> OcclusionResult:
    """Occlusion maps of `model` (a `DCRNNModel_classification`) on x (B, T, N, D): see the module docstring for the semantics.

    Per chunk of `clips_per_pass` clips: one baseline pass that keeps every layer's states; then per window k, in this order,
    `ops.occlude_expand` (the B*G variants: inputs behind t0 = k*w, the baseline's states at t0, the remaining lengths),
    `model.encoder.run` on them, `ops.cls_head`, `ops.occlusion_scores`.  The variant buffers are allocated once per chunk at the
    size of window 0; later windows use leading views of them.  Per-clip supports are replicated to the B*G variants once per
    chunk; shared 2-D supports pass through untouched.  No device-to-host synchronisation happens inside a pass; the model's mode
    is put back; no generator is drawn from.  A wrong rank or dtype of x, D % 4, misalignment, a node_groups of another shape, dtype
    or device, time_window < 1, G outside 1..64, more than 4 layers and a target for a one-output head raise ValueError before
    any launch."""
    x, groups, layers, classes = _check_inputs(model, x, seq_lengths, supports, time_window, node_groups, target, clips_per_pass)
    b_all, t_len, n, d = (int(v) for v in x.shape)
    dev, w, h = x.device, int(time_window), int(model.rnn_units)
    if groups is None:
        groups = torch.eye(n, dtype=torch.int32, device=dev)
    groups = groups.contiguous()
    g, tw = int(groups.shape[0]), -(-t_len // w)
    supports = list(supports)
    maps = torch.empty(b_all, tw, g, dtype=torch.float32, device=dev)
    base_prob = torch.empty(b_all, dtype=torch.float32, device=dev)
    base_logits = torch.empty(b_all, classes, dtype=torch.float32, device=dev)
    target_out = torch.empty(b_all, dtype=torch.int64, device=dev) if classes > 1 else None
    var_logits = torch.empty(b_all, tw, g, classes, dtype=torch.float32, device=dev) if return_logits else None
    was_training = model.training
    model.eval()
    try:
        x_var = h0_var = len_var = None
        for i in range(0, b_all, int(clips_per_pass)):
            j = min(i + int(clips_per_pass), b_all)
            b = j - i
            xc = x[i:j]
            lens = None if seq_lengths is None else seq_lengths[i:j].contiguous()
            tgt = None if target is None else target[i:j].contiguous()
            sup = [s if s.dim() == 2 else s[i:j] for s in supports]
            hexts, last = _baseline(model, xc, sup, lens)
            logits0 = ops.cls_head(last.view(b, n, h), model.fc.weight, model.fc.bias, 0.0, None).view(b, classes)
            base_logits[i:j] = logits0
            sup_var = [s if s.dim() == 2 else s.repeat_interleave(g, dim=0) for s in sup]
            if x_var is None or x_var.shape[1] != b * g:       # (the short last chunk: its own buffers)
                x_var = torch.empty(t_len, b * g, n, d, dtype=torch.float32, device=dev)
                h0_var = torch.empty(layers, b * g, n * h, dtype=torch.float32, device=dev)
                len_var = torch.empty(b * g, dtype=torch.int64, device=dev)
            for k in range(tw):
                t0 = k * w
                xv = x_var[:t_len - t0]
                ops.occlude_expand(xc, hexts, groups, lens, t0, w, fill, xv, h0_var, len_var)
                _, _, top = model.encoder.run(xv, h0_var, sup_var, lengths=len_var, want_finals=False)
                logits = ops.cls_head(top.view(b * g, n, h), model.fc.weight, model.fc.bias, 0.0, None).view(b * g, classes)
                ops.occlusion_scores(logits, logits0, lens, tgt, k, t0, maps[i:j], base_prob[i:j], None if target_out is None else target_out[i:j])
                if var_logits is not None:
                    lv = logits.view(b, g, classes)
                    if lens is not None:                       # behind the clip's end nothing the model reads has changed
                        lv = torch.where((lens > t0)[:, None, None], lv, logits0[:, None, :])
                    var_logits[i:j, k] = lv
    finally:
        model.train(was_training)
    return OcclusionResult(maps, base_prob, base_logits, target_out, var_logits)
