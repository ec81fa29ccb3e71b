"""The `torch.ops.eeg_dcrnn.*` operator library over the C ABI (include/eeg_dcrnn.h).

Every operator of the DCRNN hot path is registered with the PyTorch dispatcher (`torch.library`):
schema, device implementation (tensors in -> C-ABI launch on torch's current stream -> tensors out),
a fake (meta) implementation for tracing, and — for the differentiable ones — the autograd formula,
which calls the matching `*_bwd` operator.  PyTorch is plumbing here (device memory, streams, autograd
bookkeeping); all arithmetic runs in the HIP kernels of libeeg_dcrnn_hip.so.  The implementations are
registered for the CUDA (= HIP on ROCm) key only: this package has no CPU path (a CPU tensor gets the
dispatcher's "no kernel for the CPU backend" error, and the C-ABI stub refuses non-GPU pointers).

Operators (namespace `eeg_dcrnn`):
    hop_polys, pack_cell, diffusion_hops, dconv (+ dconv_bwd), dcgru_layer (+ dcgru_layer_bwd),
    dcgru_decoder (+ dcgru_decoder_bwd), cls_head (+ cls_head_bwd), rng_take_, dropout_mask, gather_last, corr_graph,
    fft_features (+ fft_features_len), fft_features_pair, augment_features, window_features (+ window_features_len), corr_graph_len, corr_graph_rows_len, window_features_pair, augment_windows, corr_graph_rows, bce_logits, ce_logits, masked_loss, cls_head_loss, pack_cells, clip_adam_,
    clip_adam_dev_, teacher_flags_, augment_draw_, epoch_keys, gather_clips, gather_records, eval_scores, eval_metrics, ssl_eval_scores, ssl_eval_metrics,
    feature_moments, moments_record, scan_timeline, scan_events, event_scores, resample, edf_decode, occlude_expand, occlusion_scores, bce_logits_cw, ce_logits_cw, cls_head_loss_cw, clip_weights,
    boot_counts, boot_detection, boot_classification, boot_records.
The functions below them are the Python conveniences the modules in model/ and train_step.py call.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import DecoderDims, LayerDims

ACT_CODES = {"tanh": 0, "relu": 1, None: 1}   # the reference maps anything but 'tanh' to relu (cell.py:146)
NS = "eeg_dcrnn"
_libdef = torch.library.Library(NS, "DEF")


# OPT-IN arithmetic of the two hoisted NN GEMMs of a DCGRU layer (x-part pre-activations, input gradient): 0 = the fp32 matrix pipe
# (the default and the contract's arithmetic), 1 = three-term bf16 split (6 of 9 partial products on v_mfma_f32_16x16x32_bf16,
# fp32 accumulation; include/eeg_dcrnn.h `eeg_layer_dims.pack3`).  Set it BEFORE building / capturing a step (`set_gemm_mode`, or
# EEG_DCRNN_SPLIT_BF16=1 in the environment at import): a cell's weight pack then carries the bf16 term packs behind its fp32 part,
# and forward and backward of a step must run under the same mode.
import os as _os

GEMM_MODE = 1 if _os.environ.get("EEG_DCRNN_SPLIT_BF16", "0") not in ("", "0") else 0


def set_gemm_mode(mode: int) -> int:
    """0 = fp32 MFMA (default), 1 = three-term bf16 split of the hoisted NN GEMMs (64 units; other sizes keep fp32). Returns the
    previous mode."""
    global GEMM_MODE
    if mode not in (0, 1):
        raise ValueError("gemm mode must be 0 (fp32 MFMA) or 1 (three-term bf16 split)")
    prev, GEMM_MODE = GEMM_MODE, int(mode)
    return prev


def _pack3_halves(fin, h, m) -> int:
    return int(_lib.get_lib().query("eeg_dcrnn_pack3_halves", int(fin), int(h), int(m))) if GEMM_MODE else 0


def _pack_base_floats(fin, h, m) -> int:
    """floats of the fp32 part of a cell's pack, rounded up so that what follows is 16-byte aligned"""
    return (int(_lib.get_lib().query("eeg_dcrnn_pack_floats", int(fin), int(h), int(m))) + 3) // 4 * 4


def _set_pack3(dims, pack, fin, h, m):
    """point dims.pack3 at the bf16 term packs behind the fp32 part of `pack` -- decided by what THIS pack tensor carries (it was
    built under the mode of its forward call), not by the mode at the time of the call: a backward that runs after `set_gemm_mode`
    changed keeps the arithmetic of its forward and never addresses past the end of a pack built without the term packs."""
    base = _pack_base_floats(fin, h, m)
    halves = int(_lib.get_lib().query("eeg_dcrnn_pack3_halves", int(fin), int(h), int(m)))
    if halves > 0 and pack.numel() >= base + (halves + 1) // 2:
        dims.pack3 = pack.data_ptr() + 4 * base
    elif pack.numel() != base:
        raise RuntimeError(f"weight pack has {pack.numel()} floats, expected {base} (fp32) or {base + (halves + 1) // 2} (with the "
                           f"bf16 term packs) for input_dim={fin}, num_units={h}, num_matrices={m}")


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t: torch.Tensor):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return ctypes.c_void_p(0)


def _check(lib, t: torch.Tensor, name: str, dtype=torch.float32):
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if lib.is_device_build and not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device "
                           f"and has no CPU path")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")


def _check_polys(p: torch.Tensor, p_batched: int, b: int, n: int, m: int, what: str = "P"):
    """hop-polynomial tensor of `ops.hop_polys`: (G, M-1, N, N) with G = B (per-clip graphs) or 1 (shared) -- the kernels index it
    with exactly these extents, so a tensor built for another node count / batch / hop count is refused here, not read out of bounds"""
    want = (b if p_batched else 1, m - 1, n, n)
    if m > 1 and tuple(p.shape) != want:
        raise RuntimeError(f"{what} has shape {tuple(p.shape)}, expected {want} (graphs, hop matrices - 1, num_nodes, num_nodes)")


def _check_lengths(lengths: torch.Tensor, b: int):
    if lengths.numel() != b:
        raise RuntimeError(f"seq_lengths has {lengths.numel()} entries for a batch of {b}")


def _clip_lengths(what: str, lengths: torch.Tensor, b: int, ref: torch.Tensor):
    """`lengths` of the length-aware data-side operators: read by the kernels ON THE DEVICE, so no conversion happens here -- anything
    but an int64 (B,) tensor on the device of the clips is refused"""
    if lengths.dtype != torch.int64 or tuple(lengths.shape) != (b,) or lengths.device != ref.device:
        raise RuntimeError(f"{what}: lengths must be an int64 tensor of shape ({b},) on {ref.device} (valid steps per clip, read on the "
                           f"device), got {lengths.dtype} {tuple(lengths.shape)} on {lengths.device}")
    return lengths.contiguous()


def _clip_weights(what: str, clip_w: torch.Tensor, denom: torch.Tensor, b: int, ref: torch.Tensor, name: str = "clip_w"):
    """`clip_w` / `denom` of the weighted criteria (written by `gather_clips(..., clip_w=, denom=, n_valid=)`; name "clip_u": the
    multipliers of `clip_weights`), read by the kernels ON THE DEVICE: anything but a float32 (B,) tensor and one float32 on the device
    of the clips is refused"""
    if not torch.is_tensor(clip_w) or clip_w.dtype != torch.float32 or tuple(clip_w.shape) != (b,) or clip_w.device != ref.device:
        got = f"{clip_w.dtype} {tuple(clip_w.shape)} on {clip_w.device}" if torch.is_tensor(clip_w) else type(clip_w).__name__
        raise RuntimeError(f"{what}: {name} must be a float32 tensor of shape ({b},) on {ref.device} (one weight per clip, read on the "
                           f"device), got {got}")
    if not torch.is_tensor(denom) or denom.dtype != torch.float32 or denom.numel() != 1 or denom.device != ref.device:
        got = f"{denom.dtype} {tuple(denom.shape)} on {denom.device}" if torch.is_tensor(denom) else type(denom).__name__
        raise RuntimeError(f"{what}: denom must be one float32 on {ref.device} (the divisor of the mean, read on the device), got {got}")
    return clip_w.contiguous(), denom.contiguous()


def _new(shape, like: torch.Tensor, dtype=torch.float32):
    """THE allocation of the device implementations (outputs, saved tensors, workspaces): uninitialised memory on like's device"""
    return torch.empty(shape, dtype=dtype, device=like.device)


def _new_like(t: torch.Tensor):
    """as `_new`, with the shape and dtype of the contiguous tensor t"""
    return _new(t.shape, t, t.dtype)


def _none_if_empty(t: Optional[torch.Tensor]):
    return None if (t is None or t.numel() == 0) else t


_impls = {}       # operator name -> device implementation (read by tests/emu_support.py, which drives the same
#                   implementations through the emulator build of the kernel sources)


def _tensor_device(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                return a.device
        elif isinstance(a, (list, tuple)):
            d = _tensor_device(a)
            if d is not None:
                return d
    return None


def _device_guarded(impl):
    """Python-registered operators get no DeviceGuard from the dispatcher: a call on tensors of cuda:1 while cuda:0 is the current
    device would allocate and launch on the wrong GPU.  (One process per GPU -- the layout this package is built for -- never takes
    the slow branch: one integer comparison per call.)"""
    def run(*args, **kwargs):
        dev = _tensor_device(args) or _tensor_device(tuple(kwargs.values()))
        if dev is None or dev.index is None or dev.index == torch.cuda.current_device():
            return impl(*args, **kwargs)
        with torch.cuda.device(dev):
            return impl(*args, **kwargs)
    run.__name__ = getattr(impl, "__name__", "impl")
    return run


def _define(name: str, schema: str, impl, fake):
    """schema + device implementation (CUDA key = HIP) + fake implementation."""
    _libdef.define(f"{name}{schema}")
    _libdef.impl(name, _device_guarded(impl), "CUDA")
    _impls[name] = impl
    torch.library.register_fake(f"{NS}::{name}", fake, lib=_libdef)


def _zero_impl(t) -> None:
    """t <- 0 as ONE memset on the stream (no framework fill kernel in the captured step)"""
    lib = _lib.get_lib()
    if not t.is_contiguous():
        raise RuntimeError("zero_: tensor must be contiguous")
    if lib.is_device_build and not t.is_cuda:
        raise RuntimeError("zero_: eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    lib.call("eeg_dcrnn_zero", _p(t), t.numel() * t.element_size(), _stream(t))


_define("zero_", "(Tensor(a!) t) -> ()", _zero_impl, lambda t: None)


def zero_(t: torch.Tensor) -> torch.Tensor:
    torch.ops.eeg_dcrnn.zero_(t)
    return t


def num_matrices(filter_type: str, max_diffusion_step: int) -> int:
    """cell.py:35,151-158."""
    return (2 if filter_type == "dual_random_walk" else 1) * max_diffusion_step + 1


# =============================================================================================
# hop polynomials, weight packs, the diffusion step
# =============================================================================================
def _hop_polys_impl(supports: List[torch.Tensor], max_diffusion_step: int, batch: int) -> torch.Tensor:
    lib = _lib.get_lib()
    sups = list(supports)
    if len(sups) == 0:
        raise RuntimeError("hop_polys: empty supports list")
    batched = any(s.dim() == 3 for s in sups)
    n = sups[0].shape[-1]
    norm = []
    for i, s in enumerate(sups):
        if s.shape[-1] != n or s.shape[-2] != n:
            raise RuntimeError(f"supports[{i}] has shape {tuple(s.shape)}, expected (..., {n}, {n})")
        if s.dim() == 3 and s.shape[0] != batch:
            raise RuntimeError(f"supports[{i}] batch {s.shape[0]} != input batch {batch}")
        if batched and s.dim() == 2:
            s = s.unsqueeze(0).expand(batch, n, n)
        s = s.to(torch.float32).contiguous()
        _check(lib, s, f"supports[{i}]")
        norm.append(s)
    g = batch if batched else 1
    out = _new((g, len(norm) * max_diffusion_step, n, n), norm[0])
    arr = (ctypes.c_void_p * len(norm))(*[s.data_ptr() for s in norm])
    lib.call("eeg_dcrnn_hop_polys", arr, len(norm), g, n, max_diffusion_step, _p(out), _stream(out))
    return out


def _hop_polys_fake(supports, max_diffusion_step, batch):
    g = batch if any(s.dim() == 3 for s in supports) else 1
    n = supports[0].shape[-1]
    return supports[0].new_empty((g, len(supports) * max_diffusion_step, n, n), dtype=torch.float32)


_define("hop_polys", "(Tensor[] supports, int max_diffusion_step, int batch) -> Tensor", _hop_polys_impl, _hop_polys_fake)


def _pack_cell_impl(wg, bg, wc, bc, fin: int, h: int, m: int) -> torch.Tensor:
    lib = _lib.get_lib()
    tensors = [wg.detach(), bg.detach(), wc.detach(), bc.detach()]
    for t, nm in zip(tensors, ("dconv_gate.weight", "dconv_gate.biases", "dconv_candidate.weight", "dconv_candidate.biases")):
        _check(lib, t, nm)
    rows = (fin + h) * m
    if tuple(wg.shape) != (rows, 2 * h) or tuple(wc.shape) != (rows, h) or tuple(bg.shape) != (2 * h,) or tuple(bc.shape) != (h,):
        raise RuntimeError(f"cell parameter shapes {tuple(wg.shape)}, {tuple(bg.shape)}, {tuple(wc.shape)}, {tuple(bc.shape)} "
                           f"do not match input_dim={fin}, num_units={h}, num_matrices={m}")
    base = _pack_base_floats(fin, h, m)
    halves = _pack3_halves(fin, h, m)
    pack = _new((base + (halves + 1) // 2,), wg)
    lib.call("eeg_dcrnn_pack_cell", _p(tensors[0]), _p(tensors[1]), _p(tensors[2]), _p(tensors[3]), fin, h, m, _p(pack), _stream(pack))
    if halves > 0:      # opt-in bf16 split: the three-term packs of the x-part weights ride behind the fp32 packs
        lib.call("eeg_dcrnn_pack_cell_bf16x3", _p(tensors[0]), _p(tensors[2]), fin, h, m, ctypes.c_void_p(pack.data_ptr() + 4 * base), _stream(pack))
    return pack


def _pack_floats(fin, h, m):
    """size of a cell's weight pack for shape inference: `eeg_dcrnn_pack_floats` is a pure host computation of the library
    (make_cell_pack, csrc/kernels_pack.h), so the fake implementations ask it instead of mirroring its layout"""
    return _pack_base_floats(fin, h, m) + (_pack3_halves(fin, h, m) + 1) // 2


_define("pack_cell", "(Tensor wg, Tensor bg, Tensor wc, Tensor bc, int fin, int h, int m) -> Tensor", _pack_cell_impl,
        lambda wg, bg, wc, bc, fin, h, m: wg.new_empty((_pack_floats(fin, h, m),)))


# ---- spectral form of the hoisted x-part for ONE shared symmetric support (include/eeg_dcrnn.h: eeg_layer_dims.spectral) ----------
# 1 (default): layers whose supports are given as ONE 2-D (N,N) tensor -- i.e. declared shared by the batch -- and turn out
# symmetric run their hoisted x-part in the eigenbasis of the support (K = Fin instead of M*Fin); 0: always the general path.
SPECTRAL_MODE = 0 if _os.environ.get("EEG_DCRNN_SPECTRAL", "1") in ("", "0") else 1
SPECTRAL_TOL = 2e-6          # largest |S - U diag(lam) U^T| (relative to max |S|) for which a support counts as symmetric


def set_spectral_mode(mode: int) -> int:
    """0 = general path everywhere, 1 = spectral form for shared symmetric supports (default).  Returns the previous mode."""
    global SPECTRAL_MODE
    prev, SPECTRAL_MODE = SPECTRAL_MODE, 1 if mode else 0
    return prev


def _spectral_basis_impl(support) -> torch.Tensor:
    lib = _lib.get_lib()
    sup = support.to(torch.float32).contiguous()
    _check(lib, sup, "support")
    if sup.dim() != 2 or sup.shape[0] != sup.shape[1]:
        raise RuntimeError(f"spectral_basis: support has shape {tuple(sup.shape)}, expected (num_nodes, num_nodes)")
    n = sup.shape[0]
    out = _new((lib.query("eeg_dcrnn_spectral_basis_floats", n),), sup)
    lib.call("eeg_dcrnn_spectral_basis", _p(sup), n, _p(out), _stream(sup))
    return out


def _spectral_basis_floats(n):
    return int(_lib.get_lib().query("eeg_dcrnn_spectral_basis_floats", int(n)))


_define("spectral_basis", "(Tensor support) -> Tensor", _spectral_basis_impl,
        lambda support: support.new_empty((_spectral_basis_floats(support.shape[0]),), dtype=torch.float32))


def _pack_cell_spectral_impl(wg, wc, basis, fin: int, h: int, m: int, n: int) -> torch.Tensor:
    lib = _lib.get_lib()
    wg, wc = wg.detach(), wc.detach()
    for t, nm in ((wg, "dconv_gate.weight"), (wc, "dconv_candidate.weight"), (basis, "basis")):
        _check(lib, t, nm)
    rows = (fin + h) * m
    if tuple(wg.shape) != (rows, 2 * h) or tuple(wc.shape) != (rows, h) or basis.numel() != _spectral_basis_floats(n):
        raise RuntimeError(f"pack_cell_spectral: operands {tuple(wg.shape)}, {tuple(wc.shape)}, basis {tuple(basis.shape)} do not match "
                           f"input_dim={fin}, num_units={h}, num_matrices={m}, num_nodes={n}")
    size = lib.query("eeg_dcrnn_spectral_pack_floats", fin, h, m, n)
    if size == 0:
        raise RuntimeError(f"pack_cell_spectral: the spectral form exists for 64 units (got num_units={h}, input_dim={fin})")
    out = _new((size,), wg)
    lib.call("eeg_dcrnn_pack_cell_spectral", _p(wg), _p(wc), _p(basis), fin, h, m, n, _p(out), _stream(out))
    return out


_define("pack_cell_spectral", "(Tensor wg, Tensor wc, Tensor basis, int fin, int h, int m, int n) -> Tensor", _pack_cell_spectral_impl,
        lambda wg, wc, basis, fin, h, m, n: wg.new_empty((int(_lib.get_lib().query("eeg_dcrnn_spectral_pack_floats", fin, h, m, n)),)))


def _pack_cells_impl(wgs, bgs, wcs, bcs, h: int, m: int, basis, n: int):
    """the packs of all cells of an encoder in ONE launch: [pack_0 .. pack_{L-1}] + (with a basis) [spack_0 .. spack_{L-1}]"""
    lib = _lib.get_lib()
    cells = len(wgs)
    if not (cells == len(bgs) == len(wcs) == len(bcs)) or cells < 1 or cells > 4:
        raise RuntimeError(f"pack_cells: {cells} cells (1..4, one weight / bias tensor of each kind per cell)")
    wgs, bgs, wcs, bcs = ([t.detach() for t in ts] for ts in (wgs, bgs, wcs, bcs))
    fins, packs, spacks = [], [], []
    for c in range(cells):
        fin = wgs[c].shape[0] // m - h
        rows = (fin + h) * m
        for t, nm in ((wgs[c], "dconv_gate.weight"), (bgs[c], "dconv_gate.biases"), (wcs[c], "dconv_candidate.weight"), (bcs[c], "dconv_candidate.biases")):
            _check(lib, t, nm)
        if fin < 4 or tuple(wgs[c].shape) != (rows, 2 * h) or tuple(wcs[c].shape) != (rows, h) or tuple(bgs[c].shape) != (2 * h,) \
                or tuple(bcs[c].shape) != (h,):
            raise RuntimeError(f"pack_cells: cell {c} parameter shapes {tuple(wgs[c].shape)}, {tuple(bgs[c].shape)}, {tuple(wcs[c].shape)}, "
                               f"{tuple(bcs[c].shape)} do not match num_units={h}, num_matrices={m}")
        if _pack3_halves(fin, h, m) > 0:
            raise RuntimeError("pack_cells: the opt-in bf16 split packs its cells one by one (ops.pack_cell)")
        fins.append(fin)
        packs.append(_new((_pack_base_floats(fin, h, m),), wgs[c]))
        if basis is not None:
            size = lib.query("eeg_dcrnn_spectral_pack_floats", fin, h, m, n)
            if size == 0:
                raise RuntimeError(f"pack_cells: the spectral form exists for 64 units (got num_units={h}, input_dim={fin})")
            spacks.append(_new((size,), wgs[c]))
    if basis is not None:
        _check(lib, basis, "basis")
        if basis.numel() != _spectral_basis_floats(n):
            raise RuntimeError(f"pack_cells: basis {tuple(basis.shape)} is not the block of a {n}-node support")
    tab = lambda ts: (ctypes.c_void_p * cells)(*[t.data_ptr() for t in ts])      # noqa: E731
    fin_arr = (ctypes.c_int32 * cells)(*fins)
    lib.call("eeg_dcrnn_pack_cells", cells, tab(wgs), tab(bgs), tab(wcs), tab(bcs), fin_arr, h, m, tab(packs), _p(basis), n,
             tab(spacks) if basis is not None else None, _stream(packs[0]))
    return packs + spacks


def _pack_cells_fake(wgs, bgs, wcs, bcs, h, m, basis, n):
    fins = [w.shape[0] // m - h for w in wgs]
    out = [wgs[0].new_empty((_pack_floats(f, h, m),)) for f in fins]
    if basis is not None:
        out += [wgs[0].new_empty((int(_lib.get_lib().query("eeg_dcrnn_spectral_pack_floats", f, h, m, n)),)) for f in fins]
    return out


_define("pack_cells", "(Tensor[] wg, Tensor[] bg, Tensor[] wc, Tensor[] bc, int h, int m, Tensor? basis, int n) -> Tensor[]",
        _pack_cells_impl, _pack_cells_fake)


def _diffusion_hops_impl(x, p, p_batched: int, batch: int) -> torch.Tensor:
    lib = _lib.get_lib()
    _check(lib, x, "x")
    _check(lib, p, "P")
    s, n, f = x.shape
    if p.dim() != 4:
        raise RuntimeError(f"P has shape {tuple(p.shape)}, expected (graphs, hop matrices - 1, num_nodes, num_nodes)")
    m = p.shape[1] + 1
    _check_polys(p, p_batched, batch, n, m)
    if batch < 1 or s % max(batch, 1) != 0:
        raise RuntimeError(f"diffusion_hops: {s} samples are not a multiple of the batch {batch}")
    out = _new((m - 1, s, n, f), x)
    lib.call("eeg_dcrnn_diffuse_fwd", _p(x), _p(p), p_batched, s, batch, n, f, m, _p(out), _stream(x))
    return out


_define("diffusion_hops", "(Tensor x, Tensor P, int p_batched, int batch) -> Tensor", _diffusion_hops_impl,
        lambda x, p, p_batched, batch: x.new_empty((p.shape[1],) + tuple(x.shape)))


# =============================================================================================
# DiffusionGraphConv (cell.py:66-118), differentiable
# =============================================================================================
def _dconv_impl(x, p, p_batched: int, weight, biases) -> torch.Tensor:
    lib = _lib.get_lib()
    x = x.contiguous()
    w, bvec = weight.detach().contiguous(), biases.detach().contiguous()
    for t, nm in ((x, "inputs_and_state"), (p, "P"), (w, "weight"), (bvec, "biases")):
        _check(lib, t, nm)
    b, n, f = x.shape
    if p.dim() != 4:
        raise RuntimeError(f"P has shape {tuple(p.shape)}, expected (graphs, hop matrices - 1, num_nodes, num_nodes)")
    m, o = p.shape[1] + 1, w.shape[1]
    _check_polys(p, p_batched, b, n, m)
    if w.shape[0] != f * m:
        raise RuntimeError(f"weight has {w.shape[0]} rows, expected (input_dim+hid_dim)*num_matrices = {f * m}")
    if bvec.numel() != o:
        raise RuntimeError(f"biases has {bvec.numel()} entries, expected output_dim = {o}")
    out = _new((b, n, o), x)
    ws = _new((lib.query("eeg_dcrnn_dconv_fwd_ws_floats", b, n, f, m, o),), x)
    lib.call("eeg_dcrnn_dconv_fwd", _p(x), _p(p), p_batched, b, n, f, m, _p(w), _p(bvec), o, _p(out), _p(ws), _stream(x))
    return out


def _dconv_bwd_impl(dout, x, p, p_batched: int, weight, need_dx: bool):
    lib = _lib.get_lib()
    dout, x, w = dout.contiguous(), x.contiguous(), weight.detach().contiguous()
    for t, nm in ((dout, "grad_output"), (x, "inputs_and_state"), (p, "P"), (w, "weight")):
        _check(lib, t, nm)
    b, n, f = x.shape
    m, o = p.shape[1] + 1, w.shape[1]
    _check_polys(p, p_batched, b, n, m)
    if w.shape[0] != f * m or tuple(dout.shape) != (b, n, o):
        raise RuntimeError(f"dconv_bwd: weight {tuple(w.shape)} / grad_output {tuple(dout.shape)} do not match inputs {tuple(x.shape)} with {m} hop matrices")
    dx = _new((b, n, f), x) if need_dx else _new((0,), x)
    dw, db = _new((f * m, o), x), _new((o,), x)
    ws = _new((lib.query("eeg_dcrnn_dconv_bwd_ws_floats", b, n, f, m, o),), x)
    lib.call("eeg_dcrnn_dconv_bwd", _p(x), _p(p), p_batched, b, n, f, m, _p(w), o, _p(dout), _p(dx) if need_dx else None,
             _p(dw), _p(db), _p(ws), _stream(x))
    return dx, dw, db


_define("dconv", "(Tensor x, Tensor P, int p_batched, Tensor weight, Tensor biases) -> Tensor", _dconv_impl,
        lambda x, p, p_batched, weight, biases: x.new_empty((x.shape[0], x.shape[1], weight.shape[1])))
_define("dconv_bwd", "(Tensor dout, Tensor x, Tensor P, int p_batched, Tensor weight, bool need_dx) -> (Tensor, Tensor, Tensor)",
        _dconv_bwd_impl,
        lambda dout, x, p, p_batched, weight, need_dx: (x.new_empty(x.shape if need_dx else (0,)), torch.empty_like(weight),
                                                        x.new_empty((weight.shape[1],))))


def _dconv_setup(ctx, inputs, output):
    x, p, p_batched, weight, _ = inputs
    ctx.save_for_backward(x, p, weight)
    ctx.p_batched = p_batched


def _dconv_backward(ctx, dout):
    x, p, weight = ctx.saved_tensors
    dx, dw, db = torch.ops.eeg_dcrnn.dconv_bwd(dout, x, p, ctx.p_batched, weight, ctx.needs_input_grad[0])
    return (dx if ctx.needs_input_grad[0] else None), None, None, dw, db


torch.library.register_autograd(f"{NS}::dconv", _dconv_backward, setup_context=_dconv_setup, lib=_libdef)


# =============================================================================================
# one DCGRU layer over a whole sequence (model.py:93-96 around cell.py:182-210)
# =============================================================================================
class GradSink:
    """Lets the backward operators write parameter gradients straight into caller-owned buffers (TrainStep's flat gradient
    bucket) instead of returning fresh tensors that autograd then adds into `p.grad` with one small kernel per parameter.

    No process-global state: the sink belongs to the object that owns the buffers (train_step.FlatParameters creates one and
    attaches it to each of ITS parameters as `param._eeg_grad_sink = (sink, index)`); a backward formula finds it through the
    parameter it was handed.  It is armed only inside `with sink: ...` (one backward pass); a parameter that receives a second
    gradient in the same pass falls back to the returned-tensor path (autograd accumulates), so results never depend on it."""

    def __init__(self, params: Sequence[torch.Tensor]):
        self.params = list(params)
        self.armed = False
        self.written = [False] * len(self.params)
        for i, p in enumerate(self.params):
            p._eeg_grad_sink = (self, i)

    def __enter__(self):
        self.armed = True
        self.written = [False] * len(self.params)
        return self

    def __exit__(self, *exc):
        self.armed = False
        return False

    @staticmethod
    def take(param: torch.Tensor) -> Optional[torch.Tensor]:
        """the buffer to write `param`'s gradient into, or None (-> allocate and return it to autograd)"""
        ref = getattr(param, "_eeg_grad_sink", None)
        if ref is None:
            return None
        sink, i = ref
        tgt = param.grad
        if (not sink.armed or sink.written[i] or sink.params[i] is not param or tgt is None or not tgt.is_contiguous()
                or tgt.shape != param.shape):
            return None
        sink.written[i] = True
        return tgt


def _layer_dims(t_len, b, n, h, fin, m, act, p_batched, planes_ready):
    dims = LayerDims(t_len, b, n, h, fin, m, act, p_batched)
    if planes_ready:           # the layer below's Hplanes (M-1, T+1, B, N, Fin): slots 1..T are P_m x
        dims.x_planes_ready = 1
        dims.x_plane_stride = (t_len + 1) * b * n * fin
    return dims


def _dcgru_layer_impl(x, x_off: int, h0, p, p_batched: int, wg, bg, wc, bc, lengths, x_planes, n: int, h: int, m: int,
                      act: int, save: bool, want_hsel: bool, basis=None, pack=None, spack=None):
    """x: (T + x_off, B, N, Fin) — x_off = 1 when x is the `hext` of the layer below (its slot 0 is that layer's
    initial state), whose `hpl` output is then passed as x_planes.  Returns hext (T+1, B, N*H) (slot 0 = initial
    state, slot t+1 = h_t), hsel (B, N*H) = h at t = lengths-1 (T-1 without lengths) and the tensors the backward
    needs: [xtm, pack, planes, rs, us, cs, rhs, hpl, rhpl, spack] (numel-0 placeholders where nothing is kept).
    basis (`spectral_basis` of the ONE symmetric support all clips share; p_batched must be 0): the hoisted x-part runs in the
    eigenbasis of the support; `planes` is then the node-major transformed input (N, Sp, Fin) and spack the per-frequency packs.
    pack / spack: the packs of this cell made ahead (`pack_cells`: all layers in one launch); None: packed here."""
    lib = _lib.get_lib()
    if x.dim() != 4 or x.shape[2] != n:
        raise RuntimeError(f"inputs have shape {tuple(x.shape)}, expected (T, B, num_nodes={n}, input_dim)")
    t_len, b, fin = x.shape[0] - x_off, x.shape[1], x.shape[3]
    if not lib.query("eeg_dcrnn_supported", n, h, fin, m):
        raise RuntimeError("eeg_gnn_ssl_amd: " + lib.last_error())
    _check_polys(p, p_batched, b, n, m)
    if lengths is not None:
        _check_lengths(lengths, b)
    if h0 is not None and h0.numel() != b * n * h:
        raise RuntimeError(f"initial_hidden_state has shape {tuple(h0.shape)}, expected ({b}, {n * h})")
    ready = x_planes is not None
    spec = basis is not None
    dims = _layer_dims(t_len, b, n, h, fin, m, act, p_batched, ready)
    if spec:
        _check(lib, basis, "basis")
        sp_rows = int(lib.query("eeg_dcrnn_spectral_rows", t_len * b))
        if ready:      # x_planes = the layer below's U^T h (N, B + Sp, Fin): rows B.. of every frequency are this layer's transformed input
            dims.x_plane_stride = (b + sp_rows) * fin
        if p_batched or basis.numel() != _spectral_basis_floats(n) or not lib.query("eeg_dcrnn_spectral_ok", ctypes.byref(dims), 0):
            raise RuntimeError("dcgru_layer: the spectral form needs one shared support (p_batched = 0) and a shape "
                               "eeg_dcrnn_spectral_ok accepts")
        if ready and tuple(x_planes.shape) != (n, b + sp_rows, fin):
            raise RuntimeError(f"x_planes has shape {tuple(x_planes.shape)}, expected {(n, b + sp_rows, fin)} (the layer below's U^T h)")
    empty = _new((0,), p)
    # a transposed view of a contiguous batch-major (B,T,N,Fin) tensor (what model.py:253 produces) is consumed
    # as it is: the diffusion kernel emits the time-major copy as a by-product
    xsrc, xtm = None, None
    bm = 0
    if not x.is_contiguous() and x_off == 0 and not ready and x.transpose(0, 1).is_contiguous():
        bm = 2 if spec else lib.query("eeg_dcrnn_batch_major_ok", ctypes.byref(dims))   # (the spectral node mix reads any row order)
    if bm:
        xsrc = x.transpose(0, 1)
        _check(lib, xsrc, "inputs")
        if bm == 2:                       # no copy at all: diffusion kernel and GEMMs read (b,t) rows through a map
            dims.x_batch_major = 1
            xk = xsrc
        else:
            xtm = _new((t_len, b, n, fin), x)
            xk = xtm
    else:
        if not x.is_contiguous():
            xtm = x.contiguous()
            x = xtm
        _check(lib, x, "inputs")
        xk = x[x_off:] if x_off else x
    if h0 is not None:
        h0 = h0.contiguous()
        _check(lib, h0, "initial_hidden_state")
    _check(lib, p, "P")
    pack_given, spack_given = pack is not None, spack is not None
    if pack is None:
        pack = torch.ops.eeg_dcrnn.pack_cell(wg, bg, wc, bc, fin, h, m)
    elif pack.numel() < _pack_base_floats(fin, h, m):
        raise RuntimeError(f"dcgru_layer: pack has {pack.numel()} floats, a cell of input_dim={fin}, num_units={h}, num_matrices={m} needs "
                           f"{_pack_base_floats(fin, h, m)}")
    _set_pack3(dims, pack, fin, h, m)
    s = t_len * b
    if spec:
        if spack is None:
            spack = torch.ops.eeg_dcrnn.pack_cell_spectral(wg, wc, basis, fin, h, m, n)
        elif spack.numel() != lib.query("eeg_dcrnn_spectral_pack_floats", fin, h, m, n):
            raise RuntimeError(f"dcgru_layer: spack has {spack.numel()} floats, expected {lib.query('eeg_dcrnn_spectral_pack_floats', fin, h, m, n)}")
        dims.spectral, dims.spack = basis.data_ptr(), spack.data_ptr()
        if ready:
            _check(lib, x_planes, "x_planes")
            planes, planes_ptr = _new((0,), p), x_planes.data_ptr() + 4 * b * fin
        else:
            planes = _new((n, sp_rows, fin), x)
            planes_ptr = planes.data_ptr()
    elif ready:
        _check(lib, x_planes, "x_planes")
        if tuple(x_planes.shape) != (m - 1, t_len + 1, b, n, fin):
            raise RuntimeError(f"x_planes has shape {tuple(x_planes.shape)}, expected {(m - 1, t_len + 1, b, n, fin)}")
        planes, planes_ptr = _new((0,), p), x_planes.data_ptr() + 4 * b * n * fin      # (its own placeholder: outputs must not alias)
    else:
        planes = _new((m - 1, s, n, fin), x)
        planes_ptr = planes.data_ptr()
    hext = _new((t_len + 1, b, n * h), x)
    if save:
        rs, us, cs, rhs = (_new((t_len, b, n * h), x) for _ in range(4))
        if spec:       # the by-products in the eigenbasis: U^T h_slot (slots 0..T; the next layer's transformed input) and U^T (r*h_{t-1})
            hpl, rhpl = _new((n, b + sp_rows, h), x), _new((n, sp_rows, h), x)
        else:
            hpl, rhpl = (_new((m - 1, t_len + 1, b, n, h), x) for _ in range(2))
    else:
        rs = us = cs = rhs = hpl = rhpl = None
    ws = _new((lib.query("eeg_dcrnn_layer_fwd_ws_floats", ctypes.byref(dims)),), x)
    lib.call("eeg_dcrnn_layer_fwd", ctypes.byref(dims), _p(xsrc if xsrc is not None else xk), _p(xtm) if (xsrc is not None and bm != 2) else None,
             _p(h0), _p(p), _p(pack), planes_ptr, _p(hext), _p(rs), _p(us), _p(cs), _p(rhs), _p(hpl), _p(rhpl), _p(ws), _stream(x))
    if lengths is not None:
        lengths = lengths.to(device=x.device, dtype=torch.int64).contiguous()
        hsel = _new((b, n * h), x)
        lib.call("eeg_dcrnn_gather_last", _p(hext[1:]), _p(lengths), t_len, b, n * h, _p(hsel), _stream(x))
    elif want_hsel:
        hsel = hext[t_len].clone()
    else:
        hsel = _new((0,), x)           # nobody reads the final state of this layer (a lower layer of the classification model)
    if not save:
        return hext, hsel, []
    # outputs must not alias each other or an input: packs handed in are kept by the autograd context from the INPUTS
    return hext, hsel, [xtm if xtm is not None else empty, _new((0,), p) if pack_given else pack, planes, rs, us, cs, rhs, hpl, rhpl,
                        _new((0,), p) if (spack_given or not spec) else spack]


def _dcgru_layer_fake(x, x_off, h0, p, p_batched, wg, bg, wc, bc, lengths, x_planes, n, h, m, act, save, want_hsel, basis=None,
                      pack=None, spack=None):
    t_len, b, fin = x.shape[0] - x_off, x.shape[1], x.shape[3]
    ne = lambda *shape: x.new_empty(shape)   # noqa: E731
    hext, hsel = ne(t_len + 1, b, n * h), (ne(b, n * h) if (want_hsel or lengths is not None) else ne(0))
    if not save:
        return hext, hsel, []
    # a non-contiguous x is copied time-major (kept for the backward) -- except the transposed view of a contiguous batch-major
    # tensor at a layer without handed-over planes where the kernels read it through a row map: exactly when the library's host-side
    # predicate eeg_dcrnn_batch_major_ok says 2 (1: the diffusion kernel emits the time-major copy, 0: torch copies; both keep xtm)
    zero_copy = False
    spec = basis is not None
    if not x.is_contiguous() and x_off == 0 and x_planes is None and x.transpose(0, 1).is_contiguous():
        dims = _layer_dims(t_len, b, n, h, fin, m, act, p_batched, False)
        zero_copy = spec or _lib.get_lib().query("eeg_dcrnn_batch_major_ok", ctypes.byref(dims)) == 2
    xtm = ne(t_len, b, n, fin) if (not x.is_contiguous() and not zero_copy) else ne(0)
    planes = ne(0) if x_planes is not None else ne(m - 1, t_len * b, n, fin)
    spack_in, spack = spack, ne(0)
    byp = [ne(m - 1, t_len + 1, b, n, h) for _ in range(2)]
    if spec:
        lib = _lib.get_lib()
        sp_rows = int(lib.query("eeg_dcrnn_spectral_rows", t_len * b))
        if x_planes is None:
            planes = ne(n, sp_rows, fin)
        if spack_in is None:
            spack = ne(int(lib.query("eeg_dcrnn_spectral_pack_floats", fin, h, m, n)))
        byp = [ne(n, b + sp_rows, h), ne(n, sp_rows, h)]
    return hext, hsel, [xtm, ne(0) if pack is not None else ne(_pack_floats(fin, h, m)), planes] + [ne(t_len, b, n * h) for _ in range(4)] + byp + [spack]


def _dcgru_layer_bwd_impl(d_hext, d_hsel, x, x_off: int, p, p_batched: int, pack, planes, x_planes, hext, rs, us, cs, rhs,
                          hpl, rhpl, lengths, has_h0: bool, n: int, h: int, m: int, act: int, need_dx: bool, need_dh0: bool,
                          dwg, dbg, dwc, dbc, basis=None, spack=None):
    """BPTT + all parameter gradients of one layer.  d_hext (T+1,B,N*H) w.r.t. hext (slot 0 is ignored), d_hsel
    (B,N*H) w.r.t. hsel.  dwg/dbg/dwc/dbc are overwritten.  Returns (dx (T + x_off, B, N, Fin) with the step
    gradients in slots x_off.., dh0 (B,N*H)) — numel-0 tensors where not requested."""
    lib = _lib.get_lib()
    t_len, b, fin = hext.shape[0] - 1, hext.shape[1], x.shape[3]
    ready = x_planes is not None
    dims = _layer_dims(t_len, b, n, h, fin, m, act, p_batched, ready)
    if not x.is_contiguous():             # the forward consumed the batch-major input through the row map (saved as the view)
        if not x.transpose(0, 1).is_contiguous():
            raise RuntimeError("dcgru_layer_bwd: x must be contiguous or the transposed view of a batch-major tensor")
        dims.x_batch_major = 1
    planes_ptr = x_planes.data_ptr() + 4 * b * n * fin if ready else planes.data_ptr()
    _set_pack3(dims, pack, fin, h, m)
    if basis is not None:                 # the forward ran the spectral form: `planes` is its node-major transformed input
        if ready:                         # ... handed over by the layer below: rows B.. of every frequency of its U^T h (N, B + Sp, Fin)
            dims.x_plane_stride = x_planes.shape[1] * fin
            planes_ptr = x_planes.data_ptr() + 4 * b * fin
        if spack is None or not lib.query("eeg_dcrnn_spectral_ok", ctypes.byref(dims), 1 if need_dx else 0):
            raise RuntimeError("dcgru_layer_bwd: the spectral form does not cover this call (input gradient of a layer whose "
                               "input width is not 64?)")
        dims.spectral, dims.spack = basis.data_ptr(), spack.data_ptr()
    state = b * n * h
    if d_hext is not None:
        d_hext = d_hext.contiguous()
        _check(lib, d_hext, "grad of hext")
    if d_hsel is not None:
        d_hsel = d_hsel.contiguous()
    d_hseq_ptr = ctypes.c_void_p(d_hext.data_ptr() + 4 * state) if d_hext is not None else None
    d_at_end = d_hsel if lengths is None else None
    d_at_len = d_hsel if lengths is not None else None
    xk_ptr = ctypes.c_void_p(x.data_ptr() + 4 * x_off * b * n * fin)
    dx = _new((t_len + x_off, b, n, fin), hext) if need_dx else _new((0,), hext)
    if need_dx and x_off:
        # x is the `hext` of the layer below: its slot 0 is that layer's INITIAL state, which this layer never reads.  The
        # kernels fill slots x_off.. only; the gradient of slot 0 is exactly zero (and must be a defined value: it flows
        # through autograd accumulation, hooks and anomaly detection)
        lib.call("eeg_dcrnn_zero", _p(dx), 4 * x_off * b * n * fin, _stream(dx))
    dx_ptr = ctypes.c_void_p(dx.data_ptr() + 4 * x_off * b * n * fin) if need_dx else None
    dh0 = _new((b, n * h), hext) if (need_dh0 and has_h0) else _new((0,), hext)
    ws = _new((lib.query("eeg_dcrnn_layer_bwd_ws_floats", ctypes.byref(dims), 1 if need_dx else 0),), hext)
    lib.call("eeg_dcrnn_layer_bwd", ctypes.byref(dims), xk_ptr, _p(p), _p(pack), planes_ptr, _p(hext), _p(rs),
             _p(us), _p(cs), _p(rhs), _p(_none_if_empty(hpl)), _p(_none_if_empty(rhpl)), d_hseq_ptr, _p(d_at_end), _p(d_at_len), _p(lengths), dx_ptr,
             _p(dh0) if dh0.numel() else None, _p(dwg), _p(dbg), _p(dwc), _p(dbc), _p(ws), _stream(hext))
    return dx, dh0


def _dcgru_layer_bwd_fake(d_hext, d_hsel, x, x_off, p, p_batched, pack, planes, x_planes, hext, rs, us, cs, rhs, hpl, rhpl,
                          lengths, has_h0, n, h, m, act, need_dx, need_dh0, dwg, dbg, dwc, dbc, basis=None, spack=None):
    t_len, b, fin = hext.shape[0] - 1, hext.shape[1], x.shape[3]
    return (hext.new_empty((t_len + x_off, b, n, fin) if need_dx else (0,)),
            hext.new_empty((b, n * h) if (need_dh0 and has_h0) else (0,)))


_define("dcgru_layer",
        "(Tensor x, int x_off, Tensor? h0, Tensor P, int p_batched, Tensor wg, Tensor bg, Tensor wc, Tensor bc, Tensor? lengths, "
        "Tensor? x_planes, int n, int h, int m, int act, bool save, bool want_hsel, Tensor? basis, Tensor? pack=None, Tensor? spack=None) -> "
        "(Tensor hext, Tensor hsel, Tensor[] saved)",
        _dcgru_layer_impl, _dcgru_layer_fake)
_define("dcgru_layer_bwd",
        "(Tensor? d_hext, Tensor? d_hsel, Tensor x, int x_off, Tensor P, int p_batched, Tensor pack, Tensor planes, Tensor? x_planes, "
        "Tensor hext, Tensor rs, Tensor us, Tensor cs, Tensor rhs, Tensor hpl, Tensor rhpl, Tensor? lengths, bool has_h0, int n, int h, "
        "int m, int act, bool need_dx, bool need_dh0, Tensor(a!) dwg, Tensor(b!) dbg, Tensor(c!) dwc, Tensor(d!) dbc, "
        "Tensor? basis, Tensor? spack) -> (Tensor, Tensor)",
        _dcgru_layer_bwd_impl, _dcgru_layer_bwd_fake)


def _dcgru_layer_setup(ctx, inputs, output):
    (x, x_off, h0, p, p_batched, wg, bg, wc, bc, lengths, x_planes, n, h, m, act, save, want_hsel, basis, _pack, _spack) = inputs
    hext, _, saved = output
    ctx.set_materialize_grads(False)
    ctx.saved_ok = bool(save) and len(saved) == 10
    ctx.meta = (x_off, p_batched, n, h, m, act, h0 is not None)
    ctx.params = (wg, bg, wc, bc)
    if ctx.saved_ok:
        xtm = saved[0]
        lens = None if lengths is None else lengths.to(device=x.device, dtype=torch.int64).contiguous()
        kept = list(saved[1:])
        if _pack is not None:
            kept[0] = _pack
        if _spack is not None and basis is not None:
            kept[8] = _spack
        ctx.save_for_backward(xtm if xtm.numel() else x, p, x_planes, lens, basis, hext, *kept)


def _dcgru_layer_backward(ctx, d_hext, d_hsel, d_saved):
    if not ctx.saved_ok:
        raise RuntimeError("eeg_dcrnn::dcgru_layer was run with save=False: nothing was kept for the backward pass")
    xk, p, x_planes, lens, basis, hext, pack, planes, rs, us, cs, rhs, hpl, rhpl, spack = ctx.saved_tensors
    x_off, p_batched, n, h, m, act, has_h0 = ctx.meta
    need_dx, need_dh0 = ctx.needs_input_grad[0], has_h0 and ctx.needs_input_grad[2]
    fin = xk.shape[3]
    rows = (fin + h) * m
    shapes = ((rows, 2 * h), (2 * h,), (rows, h), (h,))
    sunk = [GradSink.take(q) for q in ctx.params]           # written in place -> nothing for autograd to add
    bufs = [t if t is not None else _new(sh, hext) for t, sh in zip(sunk, shapes)]
    dx, dh0 = torch.ops.eeg_dcrnn.dcgru_layer_bwd(d_hext, d_hsel, xk, x_off, p, p_batched, pack, planes, x_planes, hext,
                                                  rs, us, cs, rhs, hpl, rhpl, lens, has_h0, n, h, m, act, need_dx, need_dh0, *bufs,
                                                  basis, spack if basis is not None else None)
    ret = [None if t is not None else g for t, g in zip(sunk, bufs)]
    grads = (dx if need_dx else None, None, dh0 if need_dh0 else None, None, None, *ret, None, None, None, None, None, None, None, None,
             None, None, None)
    # trailing arguments a caller left at their defaults (pack, spack) are not inputs of THIS call: one gradient slot per given input
    return grads[:len(ctx.needs_input_grad)]


torch.library.register_autograd(f"{NS}::dcgru_layer", _dcgru_layer_backward, setup_context=_dcgru_layer_setup, lib=_libdef)


# =============================================================================================
# decoder (model.py:160-204) as one operator
# =============================================================================================
def _dec_dims(meta, dropout_p=0.0, teacher_on_device=False):
    t_len, b, n, h, dout, m, n_layers, act, p_batched = meta
    return DecoderDims(t_len, b, n, h, dout, m, n_layers, act, p_batched, float(dropout_p), 1 if teacher_on_device else 0)


def _teacher_arg(lib, teacher, teacher_dev, t_len):
    """the `teacher` argument of eeg_dcrnn_decoder_fwd / _bwd: (void* value, keep-alive object, flags on the device?)"""
    if teacher_dev is not None:
        _check(lib, teacher_dev, "teacher_dev", torch.int32)
        if teacher_dev.numel() != t_len:
            raise RuntimeError(f"teacher_dev: expected int32[{t_len}], got {tuple(teacher_dev.shape)}")
        return _p(teacher_dev), teacher_dev, True
    if len(teacher) > 0 and any(teacher):
        arr = (ctypes.c_int32 * t_len)(*[1 if teacher[i] else 0 for i in range(t_len)])
        return ctypes.cast(arr, ctypes.c_void_p), arr, False
    return None, None, False


def make_rng_state(device, stream_id: int = 0) -> torch.Tensor:
    """State {seed, offset} (int64[2]) of the Philox4x32-10 generator behind the fused dropout masks (csrc/common.h).  The seed
    is a function of `torch.initial_seed()` (so `torch.manual_seed` governs it like it governs `nn.Dropout`) and of `stream_id`
    (the classification head and the decoder use different ones), drawn from a DEDICATED generator: the global CPU generator
    is not advanced.  Every forward call that drops advances the offset ON THE DEVICE (a replayed HIP graph keeps drawing
    fresh masks)."""
    rank = 0
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank = torch.distributed.get_rank()           # same-seed ranks draw different masks (as their data shards differ)
    g = torch.Generator().manual_seed((torch.initial_seed() + 0x9E3779B97F4A7C15 * int(stream_id) + 0xD1B54A32D192ED03 * rank) % (1 << 63))
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
    return torch.tensor([seed, 0], dtype=torch.int64, device=device)


def _check_rng(lib, t, name):
    _check(lib, t, name, torch.int64)
    if t.numel() != 2:
        raise RuntimeError(f"{name}: expected int64[2] {{seed, offset}}, got {tuple(t.shape)}")


def _dcgru_decoder_impl(targets, h0, p, p_batched: int, wg0, bg0, wc0, bc0, wg1, bg1, wc1, bc1, wp, bp, teacher: List[int],
                        t_len: int, n: int, h: int, dout: int, m: int, n_layers: int, act: int, dropout_p: float, rng_used,
                        teacher_dev=None):
    """T autoregressive steps through L cells + the projection.  teacher: T ints (1 = feed targets[t] to step t+1,
    all 0 = fully autoregressive) -- or teacher_dev: the same flags as a DEVICE int32[T] tensor (`teacher_flags_`), read by the
    persistent kernel when it starts (graph-replayable curriculum learning); dropout_p > 0: nn.Dropout in front of the projection (model.py:191), masks from the
    {seed, offset} pair `rng_used` that `rng_take_` handed out for T*B*N*H/4 counters.  Returns out (T,B,N*Dout) and
    [saved, pack0, pack1]."""
    lib = _lib.get_lib()
    if dropout_p > 0:
        if rng_used is None:
            raise RuntimeError("dcgru_decoder: dropout_p > 0 needs rng_used (ops.rng_take)")
        _check_rng(lib, rng_used, "rng_used")
    for fin in (dout, h):
        if not lib.query("eeg_dcrnn_supported", n, h, fin, m):
            raise RuntimeError("eeg_gnn_ssl_amd: " + lib.last_error())
    h0 = h0.contiguous()
    b = h0.shape[1]
    wp, bp = wp.detach().contiguous(), bp.detach().contiguous()
    for t, nm in ((h0, "initial_hidden_state"), (p, "P"), (wp, "projection_layer.weight"), (bp, "projection_layer.bias")):
        _check(lib, t, nm)
    if tuple(wp.shape) != (dout, h) or tuple(bp.shape) != (dout,):
        raise RuntimeError(f"projection_layer shapes {tuple(wp.shape)}, {tuple(bp.shape)} do not match ({dout}, {h})")
    if tuple(h0.shape) != (n_layers, b, n * h):
        raise RuntimeError(f"initial_hidden_state has shape {tuple(h0.shape)}, expected ({n_layers}, {b}, {n * h})")
    _check_polys(p, p_batched, b, n, m)
    if targets is not None and targets.numel() != t_len * b * n * dout:
        raise RuntimeError(f"decoder inputs have shape {tuple(targets.shape)}, expected ({t_len}, {b}, {n}*{dout}) "
                           f"(T, B, num_nodes * output_dim)")
    tf_ptr, tf_keep, tf_dev = _teacher_arg(lib, teacher, teacher_dev, t_len)
    use_tf = tf_ptr is not None
    if use_tf:
        if targets is None:
            raise RuntimeError("teacher forcing needs the target sequence")
        targets = targets.contiguous()
        _check(lib, targets, "inputs (teacher-forcing targets)")
    pack0 = torch.ops.eeg_dcrnn.pack_cell(wg0, bg0, wc0, bc0, dout, h, m)
    pack1 = torch.ops.eeg_dcrnn.pack_cell(wg1, bg1, wc1, bc1, h, h, m) if n_layers > 1 else _new((0,), h0)
    packs = [pack0] + [pack1] * (n_layers - 1)
    dims = _dec_dims((t_len, b, n, h, dout, m, n_layers, act, p_batched), dropout_p, tf_dev)
    out = _new((t_len, b, n * dout), h0)
    saved = _new((lib.query("eeg_dcrnn_decoder_saved_floats", ctypes.byref(dims)),), h0)
    ws = _new((lib.query("eeg_dcrnn_decoder_fwd_ws_floats", ctypes.byref(dims)),), h0)
    pk_arr = (ctypes.c_void_p * n_layers)(*[q.data_ptr() for q in packs])
    lib.call("eeg_dcrnn_decoder_fwd", ctypes.byref(dims), _p(targets) if use_tf else None, tf_ptr, _p(h0), _p(p), pk_arr,
             _p(wp), _p(bp), _p(rng_used) if dropout_p > 0 else None, _p(out), _p(saved), _p(ws), _stream(h0))
    return out, [saved, pack0, pack1]


def _dcgru_decoder_bwd_impl(d_out, p, p_batched: int, saved, pack0, pack1, wp, teacher: List[int], t_len: int, n: int, h: int,
                            dout: int, m: int, n_layers: int, act: int, dropout_p: float, rng_used,
                            dwg0, dbg0, dwc0, dbc0, dwg1, dbg1, dwc1, dbc1, dwp, dbp, teacher_dev=None):
    lib = _lib.get_lib()
    d_out = d_out.contiguous()
    _check(lib, d_out, "grad of the decoder output")
    b = d_out.shape[1]
    tf_ptr, tf_keep, tf_dev = _teacher_arg(lib, teacher, teacher_dev, t_len)
    dims = _dec_dims((t_len, b, n, h, dout, m, n_layers, act, p_batched), dropout_p, tf_dev)
    if dropout_p > 0:
        _check_rng(lib, rng_used, "rng_used")
    packs = [pack0] + [pack1] * (n_layers - 1)
    g0, g1 = (dwg0, dbg0, dwc0, dbc0), (dwg1, dbg1, dwc1, dbc1)
    dh0 = _new((n_layers, b, n * h), saved)
    ws = _new((lib.query("eeg_dcrnn_decoder_bwd_ws_floats", ctypes.byref(dims)),), saved)
    arr = lambda k: (ctypes.c_void_p * n_layers)(*[(g0 if l == 0 else g1)[k].data_ptr() for l in range(n_layers)])  # noqa: E731
    pk_arr = (ctypes.c_void_p * n_layers)(*[q.data_ptr() for q in packs])
    lib.call("eeg_dcrnn_decoder_bwd", ctypes.byref(dims), tf_ptr, _p(p), pk_arr, _p(wp.detach().contiguous()), _p(saved), _p(d_out),
             _p(rng_used) if dropout_p > 0 else None, _p(dh0), arr(0), arr(1), arr(2), arr(3), _p(dwp), _p(dbp), _p(ws), _stream(saved))
    return dh0


def _dec_saved_floats_fake(h0, t_len, n, h, dout, m, n_layers):
    return h0.new_empty((1,))        # opaque block: only the device implementation knows its size


_define("dcgru_decoder",
        "(Tensor? targets, Tensor h0, Tensor P, int p_batched, Tensor wg0, Tensor bg0, Tensor wc0, Tensor bc0, Tensor? wg1, Tensor? bg1, "
        "Tensor? wc1, Tensor? bc1, Tensor wp, Tensor bp, int[] teacher, int t_len, int n, int h, int dout, int m, int n_layers, int act, "
        "float dropout_p, Tensor? rng_used, Tensor? teacher_dev) -> (Tensor out, Tensor[] saved)",
        _dcgru_decoder_impl,
        lambda targets, h0, p, p_batched, wg0, bg0, wc0, bc0, wg1, bg1, wc1, bc1, wp, bp, teacher, t_len, n, h, dout, m, n_layers, act,
        dropout_p, rng_used, teacher_dev=None:
        (h0.new_empty((t_len, h0.shape[1], n * dout)),
         [_dec_saved_floats_fake(h0, t_len, n, h, dout, m, n_layers), h0.new_empty((_pack_floats(dout, h, m),)),
          h0.new_empty((_pack_floats(h, h, m) if n_layers > 1 else 0,))]))
_define("dcgru_decoder_bwd",
        "(Tensor d_out, Tensor P, int p_batched, Tensor saved, Tensor pack0, Tensor pack1, Tensor wp, int[] teacher, int t_len, int n, "
        "int h, int dout, int m, int n_layers, int act, float dropout_p, Tensor? rng_used, Tensor(a!) dwg0, Tensor(b!) dbg0, "
        "Tensor(c!) dwc0, Tensor(d!) dbc0, Tensor(e!)? dwg1, Tensor(f!)? dbg1, Tensor(g!)? dwc1, Tensor(h!)? dbc1, Tensor(i!) dwp, "
        "Tensor(j!) dbp, Tensor? teacher_dev) -> Tensor",
        _dcgru_decoder_bwd_impl,
        lambda d_out, p, p_batched, saved, pack0, pack1, wp, teacher, t_len, n, h, dout, m, n_layers, act, dropout_p, rng_used, *grads:
        d_out.new_empty((n_layers, d_out.shape[1], n * h)))


def _dcgru_decoder_setup(ctx, inputs, output):
    (targets, h0, p, p_batched, wg0, bg0, wc0, bc0, wg1, bg1, wc1, bc1, wp, bp, teacher, t_len, n, h, dout, m, n_layers, act,
     dropout_p, rng_used, teacher_dev) = inputs
    _, saved = output
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(p, wp, rng_used, teacher_dev, *saved)
    ctx.params = (wg0, bg0, wc0, bc0, wg1, bg1, wc1, bc1, wp, bp)
    ctx.meta = (p_batched, list(teacher), t_len, n, h, dout, m, n_layers, act, float(dropout_p))


def _dcgru_decoder_backward(ctx, d_out, d_saved):
    p, wp, rng_used, teacher_dev, saved, pack0, pack1 = ctx.saved_tensors
    p_batched, teacher, t_len, n, h, dout, m, n_layers, act, dropout_p = ctx.meta
    if d_out is None:
        return (None,) * 25
    shapes = [None if q is None else tuple(q.shape) for q in ctx.params]
    sunk = [GradSink.take(q) if q is not None else None for q in ctx.params]
    bufs = [t if t is not None else (_new(sh, saved) if sh is not None else None) for t, sh in zip(sunk, shapes)]
    dh0 = torch.ops.eeg_dcrnn.dcgru_decoder_bwd(d_out, p, p_batched, saved, pack0, pack1, wp, teacher, t_len, n, h, dout, m,
                                                n_layers, act, dropout_p, rng_used if dropout_p > 0 else None, *bufs, teacher_dev)
    ret = [None if (t is not None or g is None) else g for t, g in zip(sunk, bufs)]   # sunk: already in the caller's buffer
    return (None, dh0, None, None, *ret, None, None, None, None, None, None, None, None, None, None, None)


torch.library.register_autograd(f"{NS}::dcgru_decoder", _dcgru_decoder_backward, setup_context=_dcgru_decoder_setup, lib=_libdef)


# =============================================================================================
# heads, gather, graph construction, featurisation
# =============================================================================================
def _cls_head_impl(z, w, bias, dropout_p: float, rng_used):
    lib = _lib.get_lib()
    z, w, bias = z.contiguous(), w.detach().contiguous(), bias.detach().contiguous()
    for t, nm in ((z, "last_out"), (w, "fc.weight"), (bias, "fc.bias")):
        _check(lib, t, nm)
    if z.dim() != 3:
        raise RuntimeError(f"cls_head: last_out has shape {tuple(z.shape)}, expected (B, num_nodes, rnn_units)")
    b, n, h = z.shape
    c = w.shape[0]
    if tuple(w.shape) != (c, h) or bias.numel() != c:
        raise RuntimeError(f"cls_head: fc.weight {tuple(w.shape)} / fc.bias {tuple(bias.shape)} do not match rnn_units={h}")
    drop = dropout_p > 0
    if drop:
        if rng_used is None:
            raise RuntimeError("cls_head: dropout_p > 0 needs rng_used (ops.rng_take)")
        _check_rng(lib, rng_used, "rng_used")
    logits = _new((b, c), z)
    arg = _new((b, c), z, torch.int32)
    lib.call("eeg_dcrnn_cls_head_fwd", _p(z), _p(w), _p(bias), b, n, h, c, float(dropout_p), _p(rng_used) if drop else None,
             _p(logits), _p(arg), _stream(z))
    return logits, arg


def _rng_take_impl(rng_state, groups: int):
    """{seed, offset} of the device generator -> a fresh int64[2] tensor; the state's offset advances by `groups` counters on the
    stream (so a replayed HIP graph keeps drawing fresh masks)"""
    lib = _lib.get_lib()
    _check_rng(lib, rng_state, "rng_state")
    used = _new_like(rng_state)
    lib.call("eeg_dcrnn_rng_take", _p(rng_state), int(groups), _p(used), _stream(rng_state))
    return used


def _cls_head_bwd_impl(z, w, dlogits, arg, dropout_p: float, rng_used, dw, db):
    lib = _lib.get_lib()
    z, w, dlogits = z.contiguous(), w.detach().contiguous(), dlogits.contiguous()
    b, n, h = z.shape
    c = w.shape[0]
    if tuple(w.shape) != (c, h) or tuple(dlogits.shape) != (b, c) or tuple(arg.shape) != (b, c) or arg.dtype != torch.int32 \
            or tuple(dw.shape) != (c, h) or db.numel() != c:
        raise RuntimeError(f"cls_head_bwd: operands do not fit: z {tuple(z.shape)}, w {tuple(w.shape)}, dlogits {tuple(dlogits.shape)}, "
                           f"arg {tuple(arg.shape)} {arg.dtype}, dw {tuple(dw.shape)}, db {tuple(db.shape)}")
    dz = _new_like(z)
    lib.call("eeg_dcrnn_cls_head_bwd", _p(z), _p(w), _p(dlogits), _p(arg), b, n, h, w.shape[0], float(dropout_p),
             _p(rng_used) if dropout_p > 0 else None, _p(dz), _p(dw), _p(db), _stream(z))
    return dz


def _dropout_mask_impl(rng_used, n: int, dropout_p: float):
    """the mask x 1/(1-p) factors the fused kernels apply to elements 0..n-1 of a dropped tensor for the {seed, offset} pair a
    forward call reported (tests: handed to the oracle)"""
    lib = _lib.get_lib()
    _check_rng(lib, rng_used, "rng_used")
    mask = _new((n,), rng_used)
    lib.call("eeg_dcrnn_dropout_mask", _p(rng_used), n, float(dropout_p), _p(mask), _stream(rng_used))
    return mask


_define("rng_take_", "(Tensor(a!) rng_state, int groups) -> Tensor", _rng_take_impl, lambda rng_state, groups: torch.empty_like(rng_state))
_define("cls_head", "(Tensor z, Tensor w, Tensor bias, float dropout_p, Tensor? rng_used) -> (Tensor logits, Tensor arg)",
        _cls_head_impl,
        lambda z, w, bias, dropout_p, rng_used: (z.new_empty((z.shape[0], w.shape[0])), z.new_empty((z.shape[0], w.shape[0]), dtype=torch.int32)))
_define("cls_head_bwd", "(Tensor z, Tensor w, Tensor dlogits, Tensor arg, float dropout_p, Tensor? rng_used, Tensor(a!) dw, Tensor(b!) db) -> Tensor",
        _cls_head_bwd_impl, lambda z, w, dlogits, arg, dropout_p, rng_used, dw, db: torch.empty_like(z))
_define("dropout_mask", "(Tensor rng_used, int n, float dropout_p) -> Tensor", _dropout_mask_impl,
        lambda rng_used, n, dropout_p: rng_used.new_empty((n,), dtype=torch.float32))


def _cls_head_setup(ctx, inputs, output):
    z, w, bias, dropout_p, rng_used = inputs
    ctx.save_for_backward(z, w, output[1], rng_used)
    ctx.params = (w, bias)
    ctx.dropout_p = float(dropout_p)
    ctx.set_materialize_grads(False)


def _cls_head_backward(ctx, dlogits, _darg):
    z, w, arg, rng_used = ctx.saved_tensors
    if dlogits is None:
        return None, None, None, None, None
    sunk = [GradSink.take(q) for q in ctx.params]
    dw = sunk[0] if sunk[0] is not None else _new_like(w)
    db = sunk[1] if sunk[1] is not None else _new((w.shape[0],), z)
    dz = torch.ops.eeg_dcrnn.cls_head_bwd(z, w, dlogits, arg, ctx.dropout_p, rng_used if ctx.dropout_p > 0 else None, dw, db)
    return dz, (None if sunk[0] is not None else dw), (None if sunk[1] is not None else db), None, None


torch.library.register_autograd(f"{NS}::cls_head", _cls_head_backward, setup_context=_cls_head_setup, lib=_libdef)


def _cls_head_loss_impl(z, w, bias, targets, kind: int, dropout_p: float, rng_used, dw, db, clip_w=None, denom=None, multiply=False):
    """head forward + criterion + the head's backward for one optimisation step (eeg_dcrnn_cls_head_loss): returns
    (loss (1,), logits (B,C), arg (B,C) int32, dlogits (B,C), dz (B,N,H)); dw (C,H) / db (C) are overwritten.
    clip_w / denom (the operator cls_head_loss_w): over the clips that count (eeg_dcrnn_cls_head_loss_w); multiply (the operator
    cls_head_loss_cw): clip_w holds the per-clip multipliers clip_u (eeg_dcrnn_cls_head_loss_cw)."""
    lib = _lib.get_lib()
    z, w, bias = z.contiguous(), w.detach().contiguous(), bias.detach().contiguous()
    for t, nm in ((z, "head input"), (w, "fc.weight"), (bias, "fc.bias"), (dw, "fc.weight gradient"), (db, "fc.bias gradient")):
        _check(lib, t, nm)
    if z.dim() != 3:
        raise RuntimeError(f"cls_head_loss: head input has shape {tuple(z.shape)}, expected (B, num_nodes, rnn_units)")
    b, n, h = z.shape
    c = w.shape[0]
    if tuple(w.shape) != (c, h) or bias.numel() != c or tuple(dw.shape) != (c, h) or db.numel() != c or not dw.is_contiguous() or not db.is_contiguous():
        raise RuntimeError(f"cls_head_loss: fc operands {tuple(w.shape)}, {tuple(bias.shape)}, gradients {tuple(dw.shape)}, {tuple(db.shape)} do not "
                           f"fit a head input of {h} units")
    if kind == 0:
        tg = targets.to(torch.float32).contiguous().view(-1)
        _check(lib, tg, "targets")
    else:
        tg = targets.to(torch.int64).contiguous().view(-1)
        _check(lib, tg, "targets", torch.int64)
    if tg.numel() != b:
        raise RuntimeError(f"cls_head_loss: {tg.numel()} targets for {b} clips")
    drop = dropout_p > 0
    if drop:
        if rng_used is None:
            raise RuntimeError("cls_head_loss: dropout_p > 0 needs rng_used (ops.rng_take)")
        _check_rng(lib, rng_used, "rng_used")
    loss, logits, arg = _new((1,), z), _new((b, c), z), _new((b, c), z, torch.int32)
    dlogits, dz = _new((b, c), z), _new_like(z)
    ws = _new((lib.query("eeg_dcrnn_cls_head_loss_ws_floats", b, h, c),), z)
    if clip_w is None:
        lib.call("eeg_dcrnn_cls_head_loss", _p(z), _p(w), _p(bias), _p(tg), int(kind), b, n, h, c, float(dropout_p), _p(rng_used) if drop else None,
                 _p(logits), _p(arg), _p(dlogits), _p(dz), _p(dw), _p(db), _p(loss), _p(ws), _stream(z))
    else:
        clip_w, denom = _clip_weights("cls_head_loss", clip_w, denom, b, z, "clip_u" if multiply else "clip_w")
        lib.call("eeg_dcrnn_cls_head_loss_cw" if multiply else "eeg_dcrnn_cls_head_loss_w", _p(z), _p(w), _p(bias), _p(tg), int(kind), b, n, h, c, float(dropout_p), _p(rng_used) if drop else None,
                 _p(clip_w), _p(denom), _p(logits), _p(arg), _p(dlogits), _p(dz), _p(dw), _p(db), _p(loss), _p(ws), _stream(z))
    return loss, logits, arg, dlogits, dz


def _cls_head_loss_w_impl(z, w, bias, targets, kind: int, dropout_p: float, rng_used, clip_w, denom, dw, db):
    return _cls_head_loss_impl(z, w, bias, targets, kind, dropout_p, rng_used, dw, db, clip_w, denom)


def _cls_head_loss_cw_impl(z, w, bias, targets, kind: int, dropout_p: float, rng_used, clip_u, denom, dw, db):
    return _cls_head_loss_impl(z, w, bias, targets, kind, dropout_p, rng_used, dw, db, clip_u, denom, multiply=True)


def _cls_head_loss_fake(z, w, bias, targets, kind, dropout_p, rng_used, dw, db):
    b, c = z.shape[0], w.shape[0]
    return (z.new_empty((1,)), z.new_empty((b, c)), z.new_empty((b, c), dtype=torch.int32), z.new_empty((b, c)), torch.empty_like(z))


_define("cls_head_loss", "(Tensor z, Tensor w, Tensor bias, Tensor targets, int kind, float dropout_p, Tensor? rng_used, Tensor(a!) dw, Tensor(b!) db) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor)", _cls_head_loss_impl, _cls_head_loss_fake)
_define("cls_head_loss_w", "(Tensor z, Tensor w, Tensor bias, Tensor targets, int kind, float dropout_p, Tensor? rng_used, Tensor clip_w, Tensor denom, "
        "Tensor(a!) dw, Tensor(b!) db) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", _cls_head_loss_w_impl,
        lambda z, w, bias, targets, kind, dropout_p, rng_used, clip_w, denom, dw, db: _cls_head_loss_fake(z, w, bias, targets, kind, dropout_p, rng_used, dw, db))
_define("cls_head_loss_cw", "(Tensor z, Tensor w, Tensor bias, Tensor targets, int kind, float dropout_p, Tensor? rng_used, Tensor clip_u, Tensor denom, "
        "Tensor(a!) dw, Tensor(b!) db) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", _cls_head_loss_cw_impl,
        lambda z, w, bias, targets, kind, dropout_p, rng_used, clip_u, denom, dw, db: _cls_head_loss_fake(z, w, bias, targets, kind, dropout_p, rng_used, dw, db))


def _gather_last_impl(htop, lengths):
    lib = _lib.get_lib()
    htop = htop.contiguous()
    _check(lib, htop, "output")
    t_len, b, d = htop.shape
    _check_lengths(lengths, b)
    lengths = lengths.to(device=htop.device, dtype=torch.int64).contiguous()
    out = _new((b, d), htop)
    lib.call("eeg_dcrnn_gather_last", _p(htop), _p(lengths), t_len, b, d, _p(out), _stream(htop))
    return out


_define("gather_last", "(Tensor htop, Tensor lengths) -> Tensor", _gather_last_impl,
        lambda htop, lengths: htop.new_empty((htop.shape[1], htop.shape[2])))


def _corr_graph_impl(x, top_k: int, lengths=None):
    lib = _lib.get_lib()
    x = x.contiguous()
    _check(lib, x, "clips")
    if x.dim() != 4:
        raise RuntimeError(f"clips must be (B,T,N,D), got {tuple(x.shape)}")
    b, t_len, n, d = x.shape
    if lengths is not None:
        lengths = _clip_lengths("corr_graph_len", lengths, b, x)
    adj, s1, s2 = (_new((b, n, n), x) for _ in range(3))
    ws = _new((lib.query("eeg_dcrnn_corr_graph_ws_floats", b, t_len),), x)
    if lengths is None:
        lib.call("eeg_dcrnn_corr_graph", _p(x), b, t_len, n, d, int(top_k), _p(adj), _p(s1), _p(s2), _p(ws), _stream(x))
    else:
        lib.call("eeg_dcrnn_corr_graph_len", _p(x), b, t_len, n, d, int(top_k), _p(lengths), _p(adj), _p(s1), _p(s2), _p(ws), _stream(x))
    return adj, s1, s2


_define("corr_graph", "(Tensor x, int top_k) -> (Tensor adj, Tensor s1, Tensor s2)", _corr_graph_impl,
        lambda x, top_k: tuple(x.new_empty((x.shape[0], x.shape[2], x.shape[2])) for _ in range(3)))
# the graph of the UNPADDED clips (dataloader_classification.py:356-361): steps t >= lengths[b] of clip b do not enter the Gram
_define("corr_graph_len", "(Tensor x, int top_k, Tensor lengths) -> (Tensor adj, Tensor s1, Tensor s2)", _corr_graph_impl,
        lambda x, top_k, lengths: tuple(x.new_empty((x.shape[0], x.shape[2], x.shape[2])) for _ in range(3)))


def _fft_features_impl(raw, window: int, mean: float, std: float, standardise: bool, perm, log_scale, lengths=None, padding_val: float = 0.0):
    lib = _lib.get_lib()
    raw = raw.contiguous()
    _check(lib, raw, "raw signals")
    if raw.dim() != 3 or raw.shape[2] % window != 0:
        raise RuntimeError(f"raw signals must be (B, N, T*{window}), got {tuple(raw.shape)}")
    b, n, total = raw.shape
    t_len = total // window
    feat_raw = _new((b, t_len, n, window // 2), raw)
    feat_std = _new_like(feat_raw) if standardise else _new((0,), raw)
    if perm is not None:
        if perm.numel() != b * n:
            raise RuntimeError(f"fft_features: perm has shape {tuple(perm.shape)}, expected ({b}, {n}) source channels")
        # Every row must be a permutation of 0..N-1 (feat_raw is written at the SOURCE slot: a row that is not one would leave slots
        # of the torch.empty allocation unwritten).  A host tensor is checked here (no device sync involved); a device tensor is the
        # output of eeg_dcrnn_augment_draw (a permutation by construction) or the caller's responsibility.
        if lib.is_device_build and perm.device.type == "cpu" and not bool((torch.sort(perm.reshape(b, n).to(torch.int64), dim=1).values
                                                    == torch.arange(n, dtype=torch.int64)).all()):
            raise RuntimeError("fft_features: every row of perm must be a permutation of 0..N-1")
        perm = perm.to(device=raw.device, dtype=torch.int32).contiguous()
    if log_scale is not None and log_scale.numel() != b:
        raise RuntimeError(f"fft_features: log_scale has {log_scale.numel()} entries for {b} clips")
    if log_scale is not None:
        log_scale = log_scale.to(device=raw.device, dtype=torch.float32).contiguous()
    if lengths is None:
        lib.call("eeg_dcrnn_fft_features", _p(raw), b, n, t_len, window, _p(perm), _p(log_scale), float(mean), float(std),
                 _p(feat_raw), _p(feat_std) if standardise else None, _stream(raw))
    else:
        lengths = _clip_lengths("fft_features_len", lengths, b, raw)
        lib.call("eeg_dcrnn_fft_features_len", _p(raw), b, n, t_len, window, _p(perm), _p(log_scale), float(mean), float(std), _p(lengths),
                 float(padding_val), _p(feat_raw), _p(feat_std) if standardise else None, _stream(raw))
    return feat_raw, feat_std


def _fft_features_fake(raw, window, mean, std, standardise, perm, log_scale):
    shape = (raw.shape[0], raw.shape[2] // window, raw.shape[1], window // 2)
    return raw.new_empty(shape), raw.new_empty(shape if standardise else (0,))


_define("fft_features", "(Tensor raw, int window, float mean, float std, bool standardise, Tensor? perm, Tensor? log_scale) -> (Tensor, Tensor)",
        _fft_features_impl, _fft_features_fake)
# variable-length clips (dataloader_classification.py:25-85,321-343): windows t >= lengths[b] are not transformed
_define("fft_features_len", "(Tensor raw, int window, float mean, float std, bool standardise, Tensor? perm, Tensor? log_scale, Tensor lengths, "
        "float padding_val) -> (Tensor, Tensor)", _fft_features_impl,
        lambda raw, window, mean, std, standardise, perm, log_scale, lengths, padding_val: _fft_features_fake(raw, window, mean, std, standardise, perm,
                                                                                                              log_scale))


def _check_draws(what, perm, log_scale, b, n, ref, permutation=False):
    """perm (B, N) / log_scale (B) operands of the paired operators: shapes checked, moved to the device of `ref`.
    permutation: a HOST perm must be a permutation per row (an output written at the source slot would otherwise keep unwritten
    slots; no device sync involved -- a device tensor is the output of eeg_dcrnn_augment_draw or the caller's responsibility)"""
    if perm is not None:
        if perm.numel() != b * n:
            raise RuntimeError(f"{what}: perm has shape {tuple(perm.shape)}, expected ({b}, {n}) source channels")
        if permutation and perm.device.type == "cpu" and ref.device.type != "cpu" and not bool(
                (torch.sort(perm.reshape(b, n).to(torch.int64), dim=1).values == torch.arange(n, dtype=torch.int64)).all()):
            raise RuntimeError(f"{what}: every row of perm must be a permutation of 0..N-1")
        perm = perm.to(device=ref.device, dtype=torch.int32).contiguous()
    if log_scale is not None:
        if log_scale.numel() != b:
            raise RuntimeError(f"{what}: log_scale has {log_scale.numel()} entries for {b} clips")
        log_scale = log_scale.to(device=ref.device, dtype=torch.float32).contiguous()
    return perm, log_scale


def _fft_features_pair_impl(raw_x, raw_y, window: int, mean: float, std: float, perm, log_scale):
    lib = _lib.get_lib()
    raw_x, raw_y = raw_x.contiguous(), raw_y.contiguous()
    _check(lib, raw_x, "raw input signals")
    _check(lib, raw_y, "raw target signals")
    if raw_x.dim() != 3 or raw_x.shape[2] % window != 0 or raw_x.shape[2] == 0:
        raise RuntimeError(f"raw input signals must be (B, N, Tx*{window}), got {tuple(raw_x.shape)}")
    b, n, total = raw_x.shape
    if raw_y.dim() != 3 or tuple(raw_y.shape[:2]) != (b, n) or raw_y.shape[2] % window != 0 or raw_y.shape[2] == 0:
        raise RuntimeError(f"raw target signals must be ({b}, {n}, Ty*{window}) like the input's clips and nodes, got {tuple(raw_y.shape)}")
    tx, ty = total // window, raw_y.shape[2] // window
    perm, log_scale = _check_draws("fft_features_pair", perm, log_scale, b, n, raw_x, permutation=True)
    feat_raw = _new((b, tx, n, window // 2), raw_x)
    x_std = _new_like(feat_raw)
    y_std = _new((b, ty, n, window // 2), raw_x)
    lib.call("eeg_dcrnn_fft_features_pair", _p(raw_x), _p(raw_y), b, n, tx, ty, int(window), _p(perm), _p(log_scale), float(mean), float(std),
             _p(feat_raw), _p(x_std), _p(y_std), _stream(raw_x))
    return feat_raw, x_std, y_std


def _fft_features_pair_fake(raw_x, raw_y, window, mean, std, perm, log_scale):
    b, n, h2 = raw_x.shape[0], raw_x.shape[1], window // 2
    sx = (b, raw_x.shape[2] // window, n, h2)
    return raw_x.new_empty(sx), raw_x.new_empty(sx), raw_x.new_empty((b, raw_y.shape[2] // window, n, h2))


_define("fft_features_pair", "(Tensor raw_x, Tensor raw_y, int window, float mean, float std, Tensor? perm, Tensor? log_scale) -> "
        "(Tensor, Tensor, Tensor)", _fft_features_pair_impl, _fft_features_pair_fake)


def _augment_features_impl(x, y, perm, log_scale, feature_std: float):
    lib = _lib.get_lib()
    x, y = x.contiguous(), y.contiguous()
    _check(lib, x, "input features")
    _check(lib, y, "target features")
    if x.dim() != 4:
        raise RuntimeError(f"input features must be (B, Tx, N, D), got {tuple(x.shape)}")
    b, tx, n, d = x.shape
    if y.dim() != 4 or y.shape[0] != b or tuple(y.shape[2:]) != (n, d):
        raise RuntimeError(f"target features must be ({b}, Ty, {n}, {d}) like the input's clips, nodes and features, got {tuple(y.shape)}")
    if perm is None or log_scale is None:
        raise RuntimeError("augment_features: needs the draws (perm and log_scale)")
    if not float(feature_std) != 0.0:
        raise RuntimeError("augment_features: feature_std must be non-zero")
    perm, log_scale = _check_draws("augment_features", perm, log_scale, b, n, x)
    # the per-clip quotient (B floats) is left to the framework: it is then the very value the expression
    # `x.gather(2, idx) + (log_scale / feature_std)[:, None, None, None]` adds, on whichever device
    shift = (log_scale / float(feature_std)).contiguous()
    x_out, y_out = _new_like(x), _new_like(y)
    lib.call("eeg_dcrnn_augment_features", _p(x), _p(y), b, tx, int(y.shape[1]), n, d, _p(perm), _p(shift), _p(x_out), _p(y_out), _stream(x))
    return x_out, y_out


_define("augment_features", "(Tensor x, Tensor y, Tensor perm, Tensor log_scale, float feature_std) -> (Tensor, Tensor)",
        _augment_features_impl, lambda x, y, perm, log_scale, feature_std: (torch.empty_like(x), torch.empty_like(y)))


# ---- time-domain inputs (the reference without --use_fft) ----------------------------------------------------------------
def _check_scale(what, scale, b, ref):
    if scale is not None:
        if scale.numel() != b:
            raise RuntimeError(f"{what}: scale has {scale.numel()} entries for {b} clips")
        scale = scale.to(device=ref.device, dtype=torch.float32).contiguous()
    return scale


def _raw_windows(what, raw, window, name, like=None):
    """(B, N, T) of raw signals (B, N, T*window); `like`: the (B, N) the target of a pair must share with its input"""
    if window < 4 or window % 4 != 0:
        raise RuntimeError(f"{what}: window={window} unsupported (positive multiple of 4)")
    if raw.dim() != 3 or raw.shape[2] % window != 0 or raw.shape[2] == 0 or (like is not None and tuple(raw.shape[:2]) != like):
        want = f"(B, N, T*{window})" if like is None else f"({like[0]}, {like[1]}, Ty*{window}) like the input's clips and nodes"
        raise RuntimeError(f"raw {name} signals must be {want}, got {tuple(raw.shape)}")
    return raw.shape[0], raw.shape[1], raw.shape[2] // window


def _window_features_impl(raw, window: int, mean: float, std: float, perm, scale, lengths=None, padding_val: float = 0.0):
    lib = _lib.get_lib()
    raw = raw.contiguous()
    _check(lib, raw, "raw signals")
    b, n, t_len = _raw_windows("window_features", raw, window, "input")
    if not float(std) != 0.0:
        raise RuntimeError("window_features: std must be non-zero")
    perm, _ = _check_draws("window_features", perm, None, b, n, raw)
    scale = _check_scale("window_features", scale, b, raw)
    out = _new((b, t_len, n, window), raw)
    if lengths is None:
        lib.call("eeg_dcrnn_window_features", _p(raw), b, n, t_len, int(window), _p(perm), _p(scale), float(mean), float(std), _p(out), _stream(raw))
    else:
        lengths = _clip_lengths("window_features_len", lengths, b, raw)
        lib.call("eeg_dcrnn_window_features_len", _p(raw), b, n, t_len, int(window), _p(perm), _p(scale), float(mean), float(std), _p(lengths),
                 float(padding_val), _p(out), _stream(raw))
    return out


_define("window_features", "(Tensor raw, int window, float mean, float std, Tensor? perm, Tensor? scale) -> Tensor", _window_features_impl,
        lambda raw, window, mean, std, perm, scale: raw.new_empty((raw.shape[0], raw.shape[2] // window, raw.shape[1], window)))
_define("window_features_len", "(Tensor raw, int window, float mean, float std, Tensor? perm, Tensor? scale, Tensor lengths, float padding_val) -> Tensor",
        _window_features_impl,
        lambda raw, window, mean, std, perm, scale, lengths, padding_val: raw.new_empty((raw.shape[0], raw.shape[2] // window, raw.shape[1], window)))


def _window_features_pair_impl(raw_x, raw_y, window: int, mean: float, std: float, perm, scale):
    lib = _lib.get_lib()
    raw_x, raw_y = raw_x.contiguous(), raw_y.contiguous()
    _check(lib, raw_x, "raw input signals")
    _check(lib, raw_y, "raw target signals")
    b, n, tx = _raw_windows("window_features_pair", raw_x, window, "input")
    _, _, ty = _raw_windows("window_features_pair", raw_y, window, "target", like=(b, n))
    if not float(std) != 0.0:
        raise RuntimeError("window_features_pair: std must be non-zero")
    perm, _ = _check_draws("window_features_pair", perm, None, b, n, raw_x)
    scale = _check_scale("window_features_pair", scale, b, raw_x)
    x_std, y_std = _new((b, tx, n, window), raw_x), _new((b, ty, n, window), raw_x)
    lib.call("eeg_dcrnn_window_features_pair", _p(raw_x), _p(raw_y), b, n, tx, ty, int(window), _p(perm), _p(scale), float(mean), float(std),
             _p(x_std), _p(y_std), _stream(raw_x))
    return x_std, y_std


_define("window_features_pair", "(Tensor raw_x, Tensor raw_y, int window, float mean, float std, Tensor? perm, Tensor? scale) -> (Tensor, Tensor)",
        _window_features_pair_impl,
        lambda raw_x, raw_y, window, mean, std, perm, scale: (raw_x.new_empty((raw_x.shape[0], raw_x.shape[2] // window, raw_x.shape[1], window)),
                                                              raw_x.new_empty((raw_x.shape[0], raw_y.shape[2] // window, raw_x.shape[1], window))))


def _augment_windows_impl(x, y, perm, scale, mean: float, std: float):
    lib = _lib.get_lib()
    x = x.contiguous()
    _check(lib, x, "input windows")
    if x.dim() != 4:
        raise RuntimeError(f"input windows must be (B, Tx, N, D), got {tuple(x.shape)}")
    b, tx, n, d = x.shape
    ty = 0
    if y is not None:
        y = y.contiguous()
        _check(lib, y, "target windows")
        if y.dim() != 4 or y.shape[0] != b or tuple(y.shape[2:]) != (n, d) or y.shape[1] == 0:
            raise RuntimeError(f"target windows must be ({b}, Ty, {n}, {d}) like the input's clips, nodes and samples, got {tuple(y.shape)}")
        ty = int(y.shape[1])
    if perm is None or scale is None:
        raise RuntimeError("augment_windows: needs the draws (perm and scale)")
    if not float(std) != 0.0:
        raise RuntimeError("augment_windows: std must be non-zero")
    perm, _ = _check_draws("augment_windows", perm, None, b, n, x)
    a = _check_scale("augment_windows", scale, b, x)
    # the two per-clip factors (B floats each) are left to the framework, like `shift` of augment_features: they are then the very
    # values the expression `x.gather(2, idx) * a[:, None, None, None] + c[:, None, None, None]` uses, on whichever device
    c = ((a - 1.0) * (float(mean) / float(std))).contiguous()
    x_out = _new_like(x)
    y_out = _new_like(y) if y is not None else _new((0,), x)
    lib.call("eeg_dcrnn_augment_windows", _p(x), _p(y), b, tx, ty, n, d, _p(perm), _p(a), _p(c), _p(x_out), _p(y_out) if y is not None else None,
             _stream(x))
    return x_out, y_out


_define("augment_windows", "(Tensor x, Tensor? y, Tensor perm, Tensor scale, float mean, float std) -> (Tensor, Tensor)", _augment_windows_impl,
        lambda x, y, perm, scale, mean, std: (torch.empty_like(x), torch.empty_like(y) if y is not None else x.new_empty((0,))))


def _corr_graph_rows_impl(x, top_k: int, lengths=None, steps: int = 0):
    """x (B, N, L) raw channel rows, or (B, T, N, D) windows whose channel rows are the T pieces of D samples; with lengths, `steps`
    = the steps of a full clip (raw rows: L = steps * samples per step; windows: T)"""
    lib = _lib.get_lib()
    x = x.contiguous()
    _check(lib, x, "clips")
    if x.dim() == 3:
        (b, n, q), p, stride = x.shape, 1, 0
    elif x.dim() == 4:
        b, p, n, q = x.shape
        stride = n * q
    else:
        raise RuntimeError(f"clips must be raw rows (B,N,L) or windows (B,T,N,D), got {tuple(x.shape)}")
    if q < 4 or q % 4 != 0:
        raise RuntimeError(f"corr_graph_rows: rows of {q} samples unsupported (positive multiple of 4)")
    if b < 1 or p < 1:
        raise RuntimeError(f"corr_graph_rows: empty batch/clip {tuple(x.shape)}")
    adj, s1, s2 = (_new((b, n, n), x) for _ in range(3))
    ws = _new((lib.query("eeg_dcrnn_corr_graph_rows_ws_floats", b, p, q),), x)
    if lengths is None:
        lib.call("eeg_dcrnn_corr_graph_rows", _p(x), b, n, p, q, stride, int(top_k), _p(adj), _p(s1), _p(s2), _p(ws), _stream(x))
    else:
        lengths = _clip_lengths("corr_graph_rows_len", lengths, b, x)
        lib.call("eeg_dcrnn_corr_graph_rows_len", _p(x), b, n, p, q, stride, int(top_k), _p(lengths), int(steps), _p(adj), _p(s1), _p(s2), _p(ws),
                 _stream(x))
    return adj, s1, s2


def _corr_graph_rows_fake(x, top_k):
    n = x.shape[1] if x.dim() == 3 else x.shape[2]
    return tuple(x.new_empty((x.shape[0], n, n)) for _ in range(3))


_define("corr_graph_rows", "(Tensor x, int top_k) -> (Tensor adj, Tensor s1, Tensor s2)", _corr_graph_rows_impl, _corr_graph_rows_fake)
_define("corr_graph_rows_len", "(Tensor x, int top_k, Tensor lengths, int steps) -> (Tensor adj, Tensor s1, Tensor s2)", _corr_graph_rows_impl,
        lambda x, top_k, lengths, steps: _corr_graph_rows_fake(x, top_k))


# =============================================================================================
# losses that seed backward, optimiser tail
# =============================================================================================
def _bce_logits_impl(logits, y, clip_w=None, denom=None, multiply=False):
    lib = _lib.get_lib()
    x = logits.contiguous().view(-1)
    yy = y.to(torch.float32).contiguous().view(-1)
    _check(lib, x, "logits")
    _check(lib, yy, "targets")
    if yy.numel() != x.numel():
        raise RuntimeError(f"bce_logits: {yy.numel()} targets for {x.numel()} logits")
    loss, dx = _new((1,), x), _new_like(x)
    if clip_w is None:
        lib.call("eeg_dcrnn_bce_logits", _p(x), _p(yy), x.numel(), _p(loss), _p(dx), _stream(x))
    else:
        clip_w, denom = _clip_weights("bce_logits", clip_w, denom, x.numel(), x, "clip_u" if multiply else "clip_w")
        lib.call("eeg_dcrnn_bce_logits_cw" if multiply else "eeg_dcrnn_bce_logits_w", _p(x), _p(yy), x.numel(), _p(clip_w), _p(denom), _p(loss), _p(dx), _stream(x))
    return loss[0], dx.view(logits.shape)


def _ce_logits_impl(logits, y, clip_w=None, denom=None, multiply=False):
    lib = _lib.get_lib()
    x = logits.contiguous()
    yy = y.to(torch.int64).contiguous()
    _check(lib, x, "logits")
    _check(lib, yy, "targets", torch.int64)
    if x.dim() != 2 or yy.numel() != x.shape[0]:
        raise RuntimeError(f"ce_logits: logits {tuple(x.shape)} need shape (B, C) and {yy.numel()} targets B entries")
    loss, dx = _new((1,), x), _new_like(x)
    if clip_w is None:
        lib.call("eeg_dcrnn_ce_logits", _p(x), _p(yy), x.shape[0], x.shape[1], _p(loss), _p(dx), _stream(x))
    else:
        clip_w, denom = _clip_weights("ce_logits", clip_w, denom, x.shape[0], x, "clip_u" if multiply else "clip_w")
        lib.call("eeg_dcrnn_ce_logits_cw" if multiply else "eeg_dcrnn_ce_logits_w", _p(x), _p(yy), x.shape[0], x.shape[1], _p(clip_w), _p(denom), _p(loss), _p(dx), _stream(x))
    return loss[0], dx


def _masked_loss_impl(pred, y, use_scaler: bool, mean: float, std: float, mask_val: float, kind: int, clip_w=None, denom=None):
    lib = _lib.get_lib()
    pr = pred.contiguous()
    t = y.to(torch.float32).contiguous()
    # the kernels read 16-byte vectors: a contiguous VIEW with an odd element offset (pred.view(-1)[1:]) is not aligned
    if pr.data_ptr() % 16:
        pr = pr.clone()
    if t.data_ptr() % 16:
        t = t.clone()
    _check(lib, pr, "y_predicted")
    _check(lib, t, "y_true")
    if pr.shape != t.shape:
        raise RuntimeError(f"y_predicted {tuple(pr.shape)} and y_true {tuple(t.shape)} differ in shape")
    loss, dp = _new((1,), pr), _new_like(pr)
    ws = _new((lib.query("eeg_dcrnn_masked_loss_ws_floats"),), pr)
    if clip_w is None:
        lib.call("eeg_dcrnn_masked_loss", _p(pr), _p(t), pr.numel(), 1 if use_scaler else 0, float(mean), float(std),
                 float(mask_val), int(kind), _p(loss), _p(dp), _p(ws), _stream(pr))
    else:
        if pr.dim() < 1 or pr.shape[0] < 1:
            raise RuntimeError(f"masked_loss: y_predicted {tuple(pr.shape)} has no leading clip dimension for clip_w")
        clip_w, denom = _clip_weights("masked_loss", clip_w, denom, pr.shape[0], pr)
        lib.call("eeg_dcrnn_masked_loss_w", _p(pr), _p(t), pr.numel(), int(pr.shape[0]), _p(clip_w), _p(denom), 1 if use_scaler else 0,
                 float(mean), float(std), float(mask_val), int(kind), _p(loss), _p(dp), _p(ws), _stream(pr))
    return loss[0], dp


_loss_fake = lambda x, *a: (x.new_empty(()), torch.empty_like(x))   # noqa: E731
_define("bce_logits", "(Tensor logits, Tensor y) -> (Tensor loss, Tensor dlogits)", _bce_logits_impl, _loss_fake)
_define("ce_logits", "(Tensor logits, Tensor y) -> (Tensor loss, Tensor dlogits)", _ce_logits_impl, _loss_fake)
_define("masked_loss", "(Tensor pred, Tensor y, bool use_scaler, float mean, float std, float mask_val, int kind) -> (Tensor loss, Tensor dpred)",
        _masked_loss_impl, _loss_fake)
# the same criteria over the clips that count: clip_w (B,) float32 and denom (1,) float32 in device memory (`gather_clips`)
_define("bce_logits_w", "(Tensor logits, Tensor y, Tensor clip_w, Tensor denom) -> (Tensor loss, Tensor dlogits)", _bce_logits_impl, _loss_fake)
_define("ce_logits_w", "(Tensor logits, Tensor y, Tensor clip_w, Tensor denom) -> (Tensor loss, Tensor dlogits)", _ce_logits_impl, _loss_fake)
_define("masked_loss_w", "(Tensor pred, Tensor y, bool use_scaler, float mean, float std, float mask_val, int kind, Tensor clip_w, Tensor denom) "
        "-> (Tensor loss, Tensor dpred)", _masked_loss_impl, _loss_fake)
# the two supervised criteria with a multiplier per clip (class / sample weights): clip_u (B,) float32 >= 0 and denom (1,) float32 in
# device memory (`clip_weights`): loss = sum(u * l) / denom, dlogits = u * g / denom; u == 0 selects the clip out
_define("bce_logits_cw", "(Tensor logits, Tensor y, Tensor clip_u, Tensor denom) -> (Tensor loss, Tensor dlogits)",
        lambda logits, y, clip_u, denom: _bce_logits_impl(logits, y, clip_u, denom, multiply=True), _loss_fake)
_define("ce_logits_cw", "(Tensor logits, Tensor y, Tensor clip_u, Tensor denom) -> (Tensor loss, Tensor dlogits)",
        lambda logits, y, clip_u, denom: _ce_logits_impl(logits, y, clip_u, denom, multiply=True), _loss_fake)


WEIGHT_NORMS = {"sum": 0, "count": 1}     # eeg_dcrnn_clip_weights `norm`


def _clip_weights_impl(labels, perm, cursor, back: int, rank: int, world: int, class_w, sample_w, norm: int, clip_u, denom) -> None:
    """the step's multipliers clip_u (B,) and their divisor denom (1,), written in place (eeg_dcrnn_clip_weights).  perm / cursor given:
    the sampler form (labels = the label pool); both None: the batch form (labels = the batch's own)."""
    lib = _lib.get_lib()
    what, dev = "clip_weights", labels.device
    if labels.dtype not in (torch.float32, torch.int64) or labels.dim() != 1 or labels.numel() < 1:
        raise RuntimeError(f"{what}: labels must be float32 (detection, 0 / 1) or int64 (classification) of shape (n,), got {labels.dtype} "
                           f"{tuple(labels.shape)}")
    _check(lib, labels, "labels", labels.dtype)
    b = clip_u.numel()
    for t, name, dtype, shape in ((clip_u, "clip_u", torch.float32, (b,)), (denom, "denom", torch.float32, (1,))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous() or b < 1:
            raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {shape if name == 'denom' else '(B,)'} on {dev}, got "
                               f"{t.dtype} {tuple(t.shape)} on {t.device}")
    if (perm is None) != (cursor is None):
        raise RuntimeError(f"{what}: perm and cursor come together (the sampler form), or neither (the batch form)")
    pooled = perm is not None
    if pooled:
        for t, name, n in ((perm, "perm", None), (cursor, "cursor", 1)):
            if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1 or (n is not None and t.numel() != n) or t.device != dev or not t.is_contiguous():
                raise RuntimeError(f"{what}: {name} must be a contiguous int64 vector{'' if n is None else ' of one element'} on {dev}, got {t.dtype} "
                                   f"{tuple(t.shape)} on {t.device}")
        if not 0 <= rank < world:
            raise RuntimeError(f"{what}: rank={rank} of world={world}")
        if back not in (0, b * world):
            raise RuntimeError(f"{what}: back={back} (0: in front of the step's gather; {b * world} = batch_size*world: behind it)")
    else:
        if labels.numel() != b:
            raise RuntimeError(f"{what}: {labels.numel()} labels for the {b} clips of clip_u (the batch form: the batch's own labels)")
        if sample_w is not None or back != 0:
            raise RuntimeError(f"{what}: sample_w / back belong to the sampler form (perm and cursor are None)")
    if norm not in (0, 1):
        raise RuntimeError(f"{what}: norm={norm} (0 = sum, 1 = count)")
    classes = 0
    if class_w is not None:
        classes = class_w.numel()
        if class_w.dtype != torch.float32 or class_w.dim() != 1 or classes < 1 or class_w.device != dev or not class_w.is_contiguous() or \
                (labels.dtype == torch.float32 and classes != 2):
            raise RuntimeError(f"{what}: class_w must be a contiguous float32 vector on {dev}, one weight per class (2 for float 0 / 1 labels), "
                               f"got {class_w.dtype} {tuple(class_w.shape)} on {class_w.device}")
    if sample_w is not None and (sample_w.dtype != torch.float32 or tuple(sample_w.shape) != (labels.numel(),) or sample_w.device != dev or
                                 not sample_w.is_contiguous()):
        raise RuntimeError(f"{what}: sample_w must be a contiguous float32 tensor of shape ({labels.numel()},) on {dev} (one weight per clip of "
                           f"the pool), got {sample_w.dtype} {tuple(sample_w.shape)} on {sample_w.device}")
    lib.call("eeg_dcrnn_clip_weights", _p(labels), labels.element_size(), _p(perm), perm.numel() if pooled else 0, labels.numel() if pooled else 0,
             _p(cursor), int(back), b, int(rank) if pooled else 0, int(world) if pooled else 1, _p(class_w), classes, _p(sample_w), int(norm),
             _p(clip_u), _p(denom), _stream(clip_u))


_define("clip_weights", "(Tensor labels, Tensor? perm, Tensor? cursor, int back, int rank, int world, Tensor? class_w, Tensor? sample_w, int norm, "
        "Tensor(a!) clip_u, Tensor(b!) denom) -> ()", _clip_weights_impl, lambda *a: None)


# ---- the evaluation pass on the device (train.py:332-431; evaluation.py: DeviceEvaluator) ----------------------------------------
EVAL_MAX_CLIPS = 1 << 20      # EEG_EVAL_MAX_CLIPS: the largest pool of one pass
EVAL_RECORD_HEAD = 16         # EEG_EVAL_RECORD_HEAD: int64 words in front of the classification confusion matrix


def _eval_tensor(what, name, t, dtype, shape, dev):
    """the operands of the evaluation operators are read / written ON THE DEVICE as they are: no conversion, anything else is refused"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, got {got}")


def _eval_classes(what, probs):
    if not torch.is_tensor(probs) or probs.dim() not in (1, 2) or probs.shape[0] < 1 or (probs.dim() == 2 and probs.shape[1] < 2):
        got = f"{tuple(probs.shape)}" if torch.is_tensor(probs) else type(probs).__name__
        raise RuntimeError(f"{what}: probs must be (P,) (detection) or (P, C) with C >= 2 (classification), got {got}")
    p, c = int(probs.shape[0]), (1 if probs.dim() == 1 else int(probs.shape[1]))
    if p > EVAL_MAX_CLIPS:
        raise RuntimeError(f"{what}: P={p} clips exceed the limit of one pass, {EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    return p, c


def _eval_scores_impl(logits, label_pool, clip_w, cursor, rank: int, world: int, probs, losses) -> None:
    lib = _lib.get_lib()
    p, c = _eval_classes("eval_scores", probs)
    _check(lib, probs, "probs")
    dev = probs.device
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.shape[1] != c or logits.shape[0] < 1:
        raise RuntimeError(f"eval_scores: logits must be (B, {c}) for probs {tuple(probs.shape)}, got "
                           f"{tuple(logits.shape) if torch.is_tensor(logits) else type(logits).__name__}")
    b = int(logits.shape[0])
    _eval_tensor("eval_scores", "logits", logits, torch.float32, (b, c), dev)
    _eval_tensor("eval_scores", "losses", losses, torch.float32, (p,), dev)
    _eval_tensor("eval_scores", "label_pool", label_pool, torch.float32 if c == 1 else torch.int64, (p,), dev)
    _eval_tensor("eval_scores", "clip_w", clip_w, torch.float32, (b,), dev)
    _eval_tensor("eval_scores", "cursor", cursor, torch.int64, (1,), dev)
    if world < 1 or not 0 <= rank < world:
        raise RuntimeError(f"eval_scores: rank={rank} of world={world}")
    lib.call("eeg_dcrnn_eval_scores", _p(logits), _p(label_pool), 4 if c == 1 else 8, _p(clip_w), _p(cursor), b, c, int(rank), int(world), p,
             _p(probs), _p(losses), _stream(probs))


def eval_metrics_buffers(num_clips: int, num_classes: int, device):
    """(ws, record) of `eval_metrics` for a pool of `num_clips` clips: int32 scratch of eeg_dcrnn_eval_metrics_ws_bytes and the int64
    record (EVAL_RECORD_HEAD words, + C*C for classification); allocated once by the caller (`DeviceEvaluator`)"""
    if not 1 <= int(num_clips) <= EVAL_MAX_CLIPS:
        raise RuntimeError(f"eval_metrics: P={num_clips} clips outside 1..{EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    c = int(num_classes)
    nbytes = int(_lib.get_lib().query("eeg_dcrnn_eval_metrics_ws_bytes", int(num_clips), c))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    return ws, torch.zeros(EVAL_RECORD_HEAD + (c * c if c > 1 else 0), dtype=torch.int64, device=device)


def _eval_metrics_impl(probs, labels, losses, search: bool, thresh: float, ws, record) -> None:
    lib = _lib.get_lib()
    p, c = _eval_classes("eval_metrics", probs)
    _check(lib, probs, "probs")
    dev = probs.device
    _eval_tensor("eval_metrics", "labels", labels, torch.float32 if c == 1 else torch.int64, (p,), dev)
    _eval_tensor("eval_metrics", "losses", losses, torch.float32, (p,), dev)
    need = (int(lib.query("eeg_dcrnn_eval_metrics_ws_bytes", p, c)) + 3) // 4
    if not torch.is_tensor(ws) or ws.dtype != torch.int32 or ws.dim() != 1 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise RuntimeError(f"eval_metrics: ws must be a contiguous int32 vector of at least {need} entries on {dev} (ops.eval_metrics_buffers)")
    _eval_tensor("eval_metrics", "record", record, torch.int64, (EVAL_RECORD_HEAD + (c * c if c > 1 else 0),), dev)
    if thresh != thresh:
        raise RuntimeError("eval_metrics: thresh is NaN")
    lib.call("eeg_dcrnn_eval_metrics", _p(probs), _p(labels), 4 if c == 1 else 8, _p(losses), p, c, 1 if search else 0, float(thresh),
             _p(ws) if ws.numel() else None, _p(record), _stream(probs))


_define("eval_scores", "(Tensor logits, Tensor label_pool, Tensor clip_w, Tensor cursor, int rank, int world, Tensor(a!) probs, "
        "Tensor(b!) losses) -> ()", _eval_scores_impl, lambda *a: None)
_define("eval_metrics", "(Tensor probs, Tensor labels, Tensor losses, bool search, float thresh, Tensor(a!) ws, Tensor(b!) record) -> ()",
        _eval_metrics_impl, lambda *a: None)


# ---- the SSL evaluation pass on the device (train_ssl.py:232-280; evaluation.py: DeviceSSLEvaluator) ------------------------------
SSL_EVAL_MAX_CLIP_ELEMS = 1 << 24     # EEG_SSL_EVAL_MAX_CLIP_ELEMS: a clip holds fewer elements than this
SSL_EVAL_RECORD_WORDS = 8             # EEG_SSL_EVAL_RECORD_WORDS: float64 words of the pass's record
SSL_EVAL_RECORD = ("n", "batches", "loss", "pool_mae", "abs_sum", "count", "bad", "empty_batches")


def _ssl_eval_pool(what, scores):
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[0] != 3 or scores.shape[1] < 1:
        got = f"{tuple(scores.shape)}" if torch.is_tensor(scores) else type(scores).__name__
        raise RuntimeError(f"{what}: scores must be (3, P) float64 (abs_sum | count | bad; ops.ssl_eval_buffers), got {got}")
    p = int(scores.shape[1])
    if p > EVAL_MAX_CLIPS:
        raise RuntimeError(f"{what}: P={p} clips exceed the limit of one pass, {EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    return p


def _ssl_eval_scores_impl(pred, target, clip_w, cursor, rank: int, world: int, use_scaler: bool, mean: float, std: float, mask_val: float,
                          scores, keep=None) -> None:
    lib = _lib.get_lib()
    p = _ssl_eval_pool("ssl_eval_scores", scores)
    _check(lib, scores, "scores", torch.float64)
    dev = scores.device
    if not torch.is_tensor(pred) or pred.dim() != 4 or pred.shape[0] < 1 or pred.numel() == 0:
        raise RuntimeError(f"ssl_eval_scores: pred must be (B, Ty, N, D), got {tuple(pred.shape) if torch.is_tensor(pred) else type(pred).__name__}")
    if not torch.is_tensor(target) or tuple(target.shape) != tuple(pred.shape):
        raise RuntimeError(f"ssl_eval_scores: pred {tuple(pred.shape)} and target "
                           f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__} differ in shape")
    b, d = int(pred.shape[0]), int(pred.shape[3])
    per = pred[0].numel()
    if d % 4 != 0:
        raise RuntimeError(f"ssl_eval_scores: D={d}: the clips are read in 16-byte pieces, D must be a multiple of 4")
    if per >= SSL_EVAL_MAX_CLIP_ELEMS:
        raise RuntimeError(f"ssl_eval_scores: a clip of {per} elements; at most {SSL_EVAL_MAX_CLIP_ELEMS - 1} (EEG_SSL_EVAL_MAX_CLIP_ELEMS)")
    _eval_tensor("ssl_eval_scores", "pred", pred, torch.float32, pred.shape, dev)
    _eval_tensor("ssl_eval_scores", "target", target, torch.float32, pred.shape, dev)
    _eval_tensor("ssl_eval_scores", "clip_w", clip_w, torch.float32, (b,), dev)
    _eval_tensor("ssl_eval_scores", "cursor", cursor, torch.int64, (1,), dev)
    if keep is not None:
        _eval_tensor("ssl_eval_scores", "keep", keep, torch.float32, (p,) + tuple(pred.shape[1:]), dev)
    for name, t in (("pred", pred), ("target", target), ("keep", keep)):
        if t is not None and t.data_ptr() % 16:
            raise RuntimeError(f"ssl_eval_scores: {name} is not 16-byte aligned (a view with an odd element offset): pass a tensor of its own")
    if world < 1 or not 0 <= rank < world:
        raise RuntimeError(f"ssl_eval_scores: rank={rank} of world={world}")
    lib.call("eeg_dcrnn_ssl_eval_scores", _p(pred), _p(target), _p(clip_w), _p(cursor), b, per, d, int(rank), int(world), p, 1 if use_scaler else 0,
             float(mean), float(std), float(mask_val), _p(scores), _p(keep), _stream(scores))


def ssl_eval_buffers(num_clips: int, device, clip_shape=None):
    """(scores, record, keep) of an SSL evaluation pass over `num_clips` clips: the (3, P) float64 per-clip buffer (abs_sum | count |
    bad, zeroed), the float64 record of SSL_EVAL_RECORD_WORDS words and -- with clip_shape = (Ty, N, D) -- the (P, Ty, N, D) buffer of
    the kept predictions (else None); allocated once by the caller (`DeviceSSLEvaluator`)"""
    if not 1 <= int(num_clips) <= EVAL_MAX_CLIPS:
        raise RuntimeError(f"ssl_eval_buffers: P={num_clips} clips outside 1..{EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    keep = None if clip_shape is None else torch.zeros((int(num_clips),) + tuple(int(v) for v in clip_shape), dtype=torch.float32, device=device)
    return (torch.zeros(3, int(num_clips), dtype=torch.float64, device=device),
            torch.zeros(SSL_EVAL_RECORD_WORDS, dtype=torch.float64, device=device), keep)


def _ssl_eval_metrics_impl(scores, group: int, record) -> None:
    lib = _lib.get_lib()
    p = _ssl_eval_pool("ssl_eval_metrics", scores)
    _check(lib, scores, "scores", torch.float64)
    _eval_tensor("ssl_eval_metrics", "record", record, torch.float64, (SSL_EVAL_RECORD_WORDS,), scores.device)
    if group < 1:
        raise RuntimeError(f"ssl_eval_metrics: groups of {group} clips (the batch size of the loss, >= 1)")
    lib.call("eeg_dcrnn_ssl_eval_metrics", _p(scores), p, int(group), _p(record), _stream(scores))


_define("ssl_eval_scores", "(Tensor pred, Tensor target, Tensor clip_w, Tensor cursor, int rank, int world, bool use_scaler, float mean, float std, "
        "float mask_val, Tensor(a!) scores, Tensor(b!)? keep) -> ()", _ssl_eval_scores_impl, lambda *a: None)
_define("ssl_eval_metrics", "(Tensor scores, int group, Tensor(a!) record) -> ()", _ssl_eval_metrics_impl, lambda *a: None)


# ---- the fit of the input scaler on the device (statistics.py: fit_scaler; csrc/kernels_moments.h) ---------------------------------
MOMENTS_RECORD_WORDS = 7              # EEG_MOMENTS_RECORD_WORDS: float64 words of the pool's record
MOMENTS_RECORD = ("clips", "count", "sum", "sumsq", "mean", "std", "bad")
MOMENTS_MAX_BATCH = 65535             # EEG_MOMENTS_MAX_BATCH
MOMENTS_MAX_CLIP_ELEMS = 1 << 31      # a clip holds fewer elements than this


def _moments_tensor(what, name, t, dtype, shape, dev):
    """the operands of the moments operators are read / written ON THE DEVICE as they are: no conversion, anything else is refused"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, got {got}")


def _moments_pool(what, scores):
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[0] != 4 or scores.shape[1] < 1 or scores.dtype != torch.float64 or \
            not scores.is_contiguous():
        got = f"{scores.dtype} {tuple(scores.shape)}" if torch.is_tensor(scores) else type(scores).__name__
        raise ValueError(f"{what}: scores must be a contiguous (4, P) float64 tensor (sum | sumsq | count | bad; ops.moments_buffers), got {got}")
    p = int(scores.shape[1])
    if p > EVAL_MAX_CLIPS:
        raise ValueError(f"{what}: P={p} clips exceed the limit of one pass, {EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    return p


def _moments_shape(raw, window: int, use_fft: bool):
    """(N, T, W, kind) of the C call for a batch `raw`: raw signals (B, N, T*window), or ready features / windows (B, T, N, D) with
    window = 0 -- always the values as given, read as one row of T steps of N*D values per clip"""
    what = "feature_moments"
    if not torch.is_tensor(raw) or raw.dtype != torch.float32 or raw.dim() not in (3, 4) or raw.numel() == 0:
        got = f"{raw.dtype} {tuple(raw.shape)}" if torch.is_tensor(raw) else type(raw).__name__
        raise ValueError(f"{what}: raw must be float32 raw signals (B, N, T*window) or features / windows (B, T, N, D), got {got}")
    if not raw.is_contiguous():
        raise ValueError(f"{what}: raw {tuple(raw.shape)} must be contiguous (the clips are read in place)")
    if raw.dim() == 4:
        if window:
            raise ValueError(f"{what}: raw {tuple(raw.shape)} holds features / windows (B, T, N, D), taken as given: window={window} has no "
                             f"meaning there (raw signals are (B, N, T*window))")
        n, t, w, kind = 1, int(raw.shape[1]), int(raw.shape[2] * raw.shape[3]), 1
        if w % 4 != 0:
            raise ValueError(f"{what}: a step of {tuple(raw.shape[2:])} = {w} values is no whole number of 16-byte pieces (N*D % 4 == 0)")
    else:
        w, kind = int(window), 0 if use_fft else 1
        if w < 4 or w % 4 != 0:
            raise ValueError(f"{what}: window={window} unsupported (a positive multiple of 4)")
        if kind == 0 and w // 4 + 1 > 64:
            raise ValueError(f"{what}: window={window} unsupported with use_fft=True (a multiple of 4, at most 252)")
        if raw.shape[2] % w != 0:
            raise ValueError(f"{what}: raw {tuple(raw.shape)} is no whole number of steps of window={w} samples per channel")
        n, t = int(raw.shape[1]), int(raw.shape[2]) // w
    if raw[0].numel() >= MOMENTS_MAX_CLIP_ELEMS:
        raise ValueError(f"{what}: a clip of {raw[0].numel()} elements; at most {MOMENTS_MAX_CLIP_ELEMS - 1}")
    if raw.shape[0] > MOMENTS_MAX_BATCH:
        raise ValueError(f"{what}: B={raw.shape[0]} clips exceed one launch (EEG_MOMENTS_MAX_BATCH = {MOMENTS_MAX_BATCH})")
    if raw.data_ptr() % 16:
        raise ValueError(f"{what}: raw is not 16-byte aligned (a view with an odd element offset): pass a tensor of its own")
    return n, t, w, kind


def _feature_moments_impl(raw, lengths, clip_w, cursor, rank: int, world: int, window: int, use_fft: bool, scores) -> None:
    lib = _lib.get_lib()
    p = _moments_pool("feature_moments", scores)
    n, t, w, kind = _moments_shape(raw, window, use_fft)
    dev, b = scores.device, int(raw.shape[0])
    if lib.is_device_build and not scores.is_cuda:
        raise ValueError(f"feature_moments: scores is on {dev}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    if raw.device != dev:
        raise ValueError(f"feature_moments: raw is on {raw.device}, scores on {dev}: one device")
    if lengths is not None:
        _moments_tensor("feature_moments", "lengths", lengths, torch.int64, (b,), dev)
    if clip_w is not None:
        _moments_tensor("feature_moments", "clip_w", clip_w, torch.float32, (b,), dev)
    if cursor is not None:
        _moments_tensor("feature_moments", "cursor", cursor, torch.int64, (1,), dev)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"feature_moments: rank={rank} of world={world}")
    nbytes = int(lib.query("eeg_dcrnn_moments_ws_bytes", b, n, t, w, kind))
    if nbytes == 0:
        raise ValueError(f"feature_moments: {lib.last_error()}")
    ws = _new((nbytes // 8,), scores, torch.float64)                   # the chunks' partial words: every word read is written first
    lib.call("eeg_dcrnn_feature_moments", _p(raw), b, n, t, w, kind, _p(lengths), _p(clip_w), _p(cursor), int(rank), int(world), p, _p(ws),
             _p(scores), _stream(scores))


def moments_buffers(num_clips: int, device):
    """(scores, record) of a scaler fit over `num_clips` clips: the (4, P) float64 per-clip buffer (sum | sumsq | count | bad, zeroed)
    and the float64 record of MOMENTS_RECORD_WORDS words; allocated once by the caller (`statistics.fit_scaler`)"""
    if not 1 <= int(num_clips) <= EVAL_MAX_CLIPS:
        raise ValueError(f"moments_buffers: P={num_clips} clips outside 1..{EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    return (torch.zeros(4, int(num_clips), dtype=torch.float64, device=device),
            torch.zeros(MOMENTS_RECORD_WORDS, dtype=torch.float64, device=device))


def _moments_record_impl(scores, record) -> None:
    lib = _lib.get_lib()
    p = _moments_pool("moments_record", scores)
    if lib.is_device_build and not scores.is_cuda:
        raise ValueError(f"moments_record: scores is on {scores.device}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    _moments_tensor("moments_record", "record", record, torch.float64, (MOMENTS_RECORD_WORDS,), scores.device)
    lib.call("eeg_dcrnn_moments_record", _p(scores), p, _p(record), _stream(scores))


_define("feature_moments", "(Tensor raw, Tensor? lengths, Tensor? clip_w, Tensor? cursor, int rank, int world, int window, bool use_fft, "
        "Tensor(a!) scores) -> ()", _feature_moments_impl, lambda *a: None)
_define("moments_record", "(Tensor scores, Tensor(a!) record) -> ()", _moments_record_impl, lambda *a: None)


# ---- whole recordings: timeline, events, event scores (scan.py: Scanner; csrc/kernels_scan.h) ----------------------------------------
SCAN_CHUNK_BINS = 2048                # EEG_SCAN_CHUNK_BINS: bins of a recording `scan_events` holds in LDS at a time
SCAN_MAX_SMOOTH_BINS = 129            # EEG_SCAN_MAX_SMOOTH_BINS
SCAN_MAX_RECORDINGS = 1 << 20         # EEG_SCAN_MAX_RECORDINGS
SCAN_RECORD_WORDS = 10                # EEG_SCAN_RECORD_WORDS: int64 words of a score record
SCAN_RECORD = ("n_ref", "n_hyp", "ref_hit", "hyp_hit", "covered_bins", "tp", "fp", "fn", "tn", "overflowed")
SCAN_AGG = {"mean": 0, "max": 1}      # eeg_dcrnn_scan_timeline `agg`


def _scan_tensor(what, name, t, dtype, shape, dev):
    """the operands of the scan operators are read / written ON THE DEVICE as they are (None in shape: any extent >= 1)"""
    ok = torch.is_tensor(t) and t.dtype == dtype and t.dim() == len(shape) and t.device == dev and t.is_contiguous() and \
        all((v >= 1) if w is None else (v == w) for v, w in zip(t.shape, shape))
    if not ok:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        want = "(" + ", ".join("*" if w is None else str(w) for w in shape) + ("," if len(shape) == 1 else "") + ")"
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {want} on {dev}, got {got}")


def _scan_bins(what, lib, bin_off, per_bin):
    """(R, total_bins, device) of a scan operator from bin_off (R + 1,) and its first per-bin tensor"""
    if not torch.is_tensor(per_bin) or per_bin.dim() != 1 or per_bin.numel() < 1:
        got = f"{tuple(per_bin.shape)}" if torch.is_tensor(per_bin) else type(per_bin).__name__
        raise ValueError(f"{what}: the per-bin tensors are (total_bins,) with total_bins >= 1 (ops.scan_buffers), got {got}")
    dev = per_bin.device
    if lib.is_device_build and not per_bin.is_cuda:
        raise ValueError(f"{what}: the tensors are on {dev}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    _scan_tensor(what, "bin_off", bin_off, torch.int64, (None,), dev)
    r = bin_off.numel() - 1
    if not 1 <= r <= SCAN_MAX_RECORDINGS:
        raise ValueError(f"{what}: bin_off has {bin_off.numel()} entries: R + 1 for 1..{SCAN_MAX_RECORDINGS} recordings")
    if per_bin.numel() >= 1 << 31:
        raise ValueError(f"{what}: total_bins={per_bin.numel()} bins; at most 2^31 - 1")
    return r, int(per_bin.numel()), dev


def _scan_timeline_impl(probs, clip_table, clip_off, bin_off, x_steps: int, window: int, agg: int, timeline, cover) -> None:
    lib = _lib.get_lib()
    what = "scan_timeline"
    r, total, dev = _scan_bins(what, lib, bin_off, timeline)
    _scan_tensor(what, "timeline", timeline, torch.float32, (total,), dev)
    _scan_tensor(what, "cover", cover, torch.int32, (total,), dev)
    _scan_tensor(what, "probs", probs, torch.float32, (None,), dev)
    p = int(probs.numel())
    if p > EVAL_MAX_CLIPS:
        raise ValueError(f"{what}: P={p} clips exceed the limit of one pass, {EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    _scan_tensor(what, "clip_table", clip_table, torch.int64, (p, 4), dev)
    _scan_tensor(what, "clip_off", clip_off, torch.int64, (r + 1,), dev)
    if x_steps < 1 or window < 1:
        raise ValueError(f"{what}: x_steps={x_steps}, window={window} (both >= 1)")
    if agg not in (0, 1):
        raise ValueError(f"{what}: agg={agg} (0 = mean, 1 = max)")
    lib.call("eeg_dcrnn_scan_timeline", _p(probs), p, _p(clip_table), _p(clip_off), _p(bin_off), r, total, int(x_steps), int(window), int(agg),
             _p(timeline), _p(cover), _stream(timeline))


def _scan_events_impl(timeline, cover, bin_off, smooth_bins: int, th_on: float, th_off: float, merge_gap: int, min_bins: int, smoothed, events,
                      event_count) -> None:
    lib = _lib.get_lib()
    what = "scan_events"
    r, total, dev = _scan_bins(what, lib, bin_off, timeline)
    _scan_tensor(what, "timeline", timeline, torch.float32, (total,), dev)
    _scan_tensor(what, "cover", cover, torch.int32, (total,), dev)
    _scan_tensor(what, "smoothed", smoothed, torch.float32, (total,), dev)
    if not torch.is_tensor(events) or events.dim() != 3 or events.shape[1] < 1:
        got = f"{tuple(events.shape)}" if torch.is_tensor(events) else type(events).__name__
        raise ValueError(f"{what}: events must be (R, E_max, 2) int32 with E_max >= 1 (E_max < 1 holds no event), got {got}")
    _scan_tensor(what, "events", events, torch.int32, (r, None, 2), dev)
    _scan_tensor(what, "event_count", event_count, torch.int32, (r,), dev)
    if smooth_bins < 1 or smooth_bins % 2 == 0 or smooth_bins > SCAN_MAX_SMOOTH_BINS:
        raise ValueError(f"{what}: smooth_bins={smooth_bins} must be odd, 1..{SCAN_MAX_SMOOTH_BINS} (a centred window; 1 = no smoothing)")
    if th_on != th_on or th_off != th_off:
        raise ValueError(f"{what}: a threshold is NaN (th_on={th_on}, th_off={th_off})")
    if th_off > th_on:
        raise ValueError(f"{what}: th_off={th_off} above th_on={th_on} (hysteresis: on at th_on, off below th_off <= th_on)")
    if merge_gap < 0 or min_bins < 1:
        raise ValueError(f"{what}: merge_gap={merge_gap} (>= 0), min_bins={min_bins} (>= 1)")
    lib.call("eeg_dcrnn_scan_events", _p(timeline), _p(cover), _p(bin_off), r, total, int(smooth_bins), float(th_on), float(th_off), int(merge_gap),
             int(min_bins), int(events.shape[1]), _p(smoothed), _p(events), _p(event_count), _stream(timeline))


def _event_scores_impl(events, event_count, ref, ref_count, cover, bin_off, record, rec_records) -> None:
    lib = _lib.get_lib()
    what = "event_scores"
    r, total, dev = _scan_bins(what, lib, bin_off, cover)
    _scan_tensor(what, "cover", cover, torch.int32, (total,), dev)
    _scan_tensor(what, "events", events, torch.int32, (r, None, 2), dev)
    _scan_tensor(what, "event_count", event_count, torch.int32, (r,), dev)
    _scan_tensor(what, "ref", ref, torch.int32, (r, None, 2), dev)
    _scan_tensor(what, "ref_count", ref_count, torch.int32, (r,), dev)
    _scan_tensor(what, "record", record, torch.int64, (SCAN_RECORD_WORDS,), dev)
    _scan_tensor(what, "rec_records", rec_records, torch.int64, (r, SCAN_RECORD_WORDS), dev)
    lib.call("eeg_dcrnn_event_scores", _p(events), _p(event_count), int(events.shape[1]), _p(ref), _p(ref_count), int(ref.shape[1]), _p(cover),
             _p(bin_off), r, total, _p(record), _p(rec_records), _stream(cover))


_define("scan_timeline", "(Tensor probs, Tensor clip_table, Tensor clip_off, Tensor bin_off, int x_steps, int window, int agg, Tensor(a!) timeline, "
        "Tensor(b!) cover) -> ()", _scan_timeline_impl, lambda *a: None)
_define("scan_events", "(Tensor timeline, Tensor cover, Tensor bin_off, int smooth_bins, float th_on, float th_off, int merge_gap, int min_bins, "
        "Tensor(a!) smoothed, Tensor(b!) events, Tensor(c!) event_count) -> ()", _scan_events_impl, lambda *a: None)
_define("event_scores", "(Tensor events, Tensor event_count, Tensor ref, Tensor ref_count, Tensor cover, Tensor bin_off, Tensor(a!) record, "
        "Tensor(b!) rec_records) -> ()", _event_scores_impl, lambda *a: None)


# ---- native-rate recordings to the model's rate (resample.py; the reference's data/resample_signals.py:38-43) -------------------------
RESAMPLE_MAX_SAMPLES = 1 << 22       # EEG_RESAMPLE_MAX_SAMPLES


def _resample_lengths(what, n_in: int, n_out: int):
    if not 2 <= n_in <= RESAMPLE_MAX_SAMPLES:
        raise ValueError(f"{what}: {n_in} input samples per channel; 2..{RESAMPLE_MAX_SAMPLES} (EEG_RESAMPLE_MAX_SAMPLES) are supported")
    if not 1 <= n_out <= RESAMPLE_MAX_SAMPLES:
        raise ValueError(f"{what}: n_out={n_out} output samples per channel; 1..{RESAMPLE_MAX_SAMPLES} (EEG_RESAMPLE_MAX_SAMPLES) are supported")


def resample_into(x, out, workspace_bytes=None, what: str = "resample"):
    """rows of x (N, L) float32 / float64 (row stride >= L) -> the rows of out (N, n_out) float32 (row stride >= n_out), both on the
    device; the workspace comes from the caching allocator, all channels at once unless `workspace_bytes` caps it (never below one
    channel's need: the channels then run in chunks, same bits).  Everything is checked before the launch."""
    lib = _lib.get_lib()
    for name, t, dtypes in (("x", x, (torch.float32, torch.float64)), ("out", out, (torch.float32,))):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype not in dtypes:
            got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{what}: {name} must be a 2-D (channels, samples) tensor of {' or '.join(str(d) for d in dtypes)}, got {got}")
        if t.shape[0] < 1 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"{what}: the rows of {name} must be contiguous with a row stride of at least the row length, got shape "
                             f"{tuple(t.shape)} with strides {tuple(t.stride())}")
    if lib.is_device_build and not x.is_cuda:
        raise ValueError(f"{what}: x is on {x.device}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    if out.device != x.device or out.shape[0] != x.shape[0]:
        raise ValueError(f"{what}: out is {tuple(out.shape)} on {out.device} for x {tuple(x.shape)} on {x.device}")
    if x.requires_grad:
        raise ValueError(f"{what}: x requires grad; resampling has no gradient formula (detach it)")
    n, n_in, n_out = int(x.shape[0]), int(x.shape[1]), int(out.shape[1])
    _resample_lengths(what, n_in, n_out)
    one = int(lib.query("eeg_dcrnn_resample_ws_bytes", n_in, n_out, 1))
    ws_bytes = int(lib.query("eeg_dcrnn_resample_ws_bytes", n_in, n_out, n))
    if one == 0 or ws_bytes == 0:
        raise ValueError(f"{what}: the library refuses {n} channels of {n_in} -> {n_out} samples")
    if workspace_bytes is not None:
        if int(workspace_bytes) < one:
            raise ValueError(f"{what}: workspace_bytes={workspace_bytes} is below the {one} bytes one channel of {n_in} -> {n_out} samples needs")
        ws_bytes = min(ws_bytes, int(workspace_bytes))
    ws = _new((ws_bytes + 15) // 16 * 2, x, torch.float64)
    lib.call("eeg_dcrnn_resample", _p(x), 1 if x.dtype == torch.float64 else 0, n, n_in, int(x.stride(0)) if n > 1 else n_in, n_out, _p(out),
             int(out.stride(0)) if n > 1 else n_out, _p(ws), ws_bytes, _stream(x))
    return out


def _resample_impl(x, n_out: int, workspace_bytes: Optional[int] = None):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"resample: x must be a 2-D (channels, samples) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if x.shape[0] >= 1:
        _resample_lengths("resample", int(x.shape[1]), int(n_out))
    return resample_into(x, _new((x.shape[0], int(n_out)), x), workspace_bytes)


def _resample_fake(x, n_out, workspace_bytes=None):
    return x.new_empty((x.shape[0], n_out), dtype=torch.float32)


_define("resample", "(Tensor x, int n_out, int? workspace_bytes=None) -> Tensor", _resample_impl, _resample_fake)


# ---- EDF recordings decoded on the device (edf.py; the reference's data/data_utils.py getEDFsignals) ---------------------------------
EDF_MAX_CHANNELS = 32       # EEG_EDF_MAX_CHANNELS
EDF_MAX_N = 1 << 30         # samples per data record of a selected signal
_EDF_DTYPES = (torch.float64, torch.float32)


def _edf_int(what, name, v, low):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < low:
        raise ValueError(f"{what}: {name}={v!r} must be an integer >= {low}")
    return int(v)


def _edf_args(what, payload, num_records, R, n, chan_off, gain, offset):
    """the checks shared by the operator, its fake implementation and `edf_decode_into`: -> (num_records, R, n, chan_off, gain, offset)"""
    if not torch.is_tensor(payload) or payload.dtype != torch.uint8 or payload.dim() != 1 or payload.stride(0) != 1:
        got = f"{payload.dtype} {tuple(payload.shape)}" if torch.is_tensor(payload) else type(payload).__name__
        raise ValueError(f"{what}: payload must be a 1-D contiguous torch.uint8 tensor (the bytes behind the EDF header), got {got}")
    num_records, R, n = _edf_int(what, "num_records", num_records, 1), _edf_int(what, "R", R, 1), _edf_int(what, "n", n, 1)
    if n > EDF_MAX_N:
        raise ValueError(f"{what}: n={n} samples per record; 1..{EDF_MAX_N} are supported")
    chan_off, gain, offset = list(chan_off), list(gain), list(offset)
    if not 1 <= len(chan_off) <= EDF_MAX_CHANNELS:
        raise ValueError(f"{what}: {len(chan_off)} channels; 1..{EDF_MAX_CHANNELS} (EEG_EDF_MAX_CHANNELS) are supported")
    if len(gain) != len(chan_off) or len(offset) != len(chan_off):
        raise ValueError(f"{what}: {len(gain)} gains and {len(offset)} offsets for {len(chan_off)} channels")
    for c, o in enumerate(chan_off):
        if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or o < 0 or o + n > R:
            raise ValueError(f"{what}: chan_off[{c}]={o!r} + n={n} lies outside a record of R={R} int16")
    for name, vals in (("gain", gain), ("offset", offset)):
        for c, v in enumerate(vals):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
                raise ValueError(f"{what}: {name}[{c}]={v!r} must be a finite number")
    if payload.numel() < 2 * num_records * R:
        raise ValueError(f"{what}: payload of {payload.numel()} bytes is shorter than num_records={num_records} whole records of R={R} int16 "
                         f"({2 * num_records * R} bytes)")
    return num_records, R, n, [int(o) for o in chan_off], [float(g) for g in gain], [float(o) for o in offset]


def edf_decode_into(payload, num_records, R, n, chan_off, gain, offset, out, what: str = "edf_decode"):
    """the selected channels of an EDF payload ON THE DEVICE -> the rows of out (C, num_records * n) float64 / float32 (row stride >= the
    row length, so `out` may be a strided view of a larger buffer): out[c, r * n + j] = gain[c] * (offset[c] + int16 at payload index
    r * R + chan_off[c] + j), float64 arithmetic, rounded once for a float32 `out`.  Everything is checked before the launch."""
    lib = _lib.get_lib()
    num_records, R, n, chan_off, gain, offset = _edf_args(what, payload, num_records, R, n, chan_off, gain, offset)
    if lib.is_device_build and not payload.is_cuda:
        raise ValueError(f"{what}: payload is on {payload.device}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    if payload.data_ptr() % 2 != 0:
        raise ValueError(f"{what}: payload starts at an odd address; the int16 samples must be 2-byte aligned")
    C, L = len(chan_off), num_records * n
    if not torch.is_tensor(out) or out.dim() != 2 or out.dtype not in _EDF_DTYPES:
        got = f"{out.dtype} {tuple(out.shape)}" if torch.is_tensor(out) else type(out).__name__
        raise ValueError(f"{what}: out must be a 2-D (channels, samples) tensor of torch.float64 or torch.float32, got {got}")
    if tuple(out.shape) != (C, L) or out.device != payload.device:
        raise ValueError(f"{what}: out is {tuple(out.shape)} on {out.device}; {C} channels of num_records * n = {L} samples on {payload.device} are decoded")
    if out.stride(1) != 1 or (C > 1 and out.stride(0) < L):
        raise ValueError(f"{what}: the rows of out must be contiguous with a row stride of at least the row length, got shape "
                         f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    lib.call("eeg_dcrnn_edf_decode", _p(payload), payload.numel(), num_records, R, n, C, (ctypes.c_int64 * C)(*chan_off), (ctypes.c_double * C)(*gain),
             (ctypes.c_double * C)(*offset), 1 if out.dtype == torch.float64 else 0, _p(out), int(out.stride(0)) if C > 1 else L, _stream(payload))
    return out


def _edf_out_dtype(what, out_dtype):
    dtype = torch.float64 if out_dtype is None else out_dtype
    if dtype not in _EDF_DTYPES:
        raise ValueError(f"{what}: out_dtype={out_dtype!r}; torch.float64 or torch.float32")
    return dtype


def _edf_decode_impl(payload, num_records, R, n, chan_off, gain, offset, out_dtype=None):
    dtype = _edf_out_dtype("edf_decode", out_dtype)
    num_records, R, n, chan_off, gain, offset = _edf_args("edf_decode", payload, num_records, R, n, chan_off, gain, offset)
    return edf_decode_into(payload, num_records, R, n, chan_off, gain, offset, _new((len(chan_off), num_records * n), payload, dtype))


def _edf_decode_fake(payload, num_records, R, n, chan_off, gain, offset, out_dtype=None):
    return payload.new_empty((len(chan_off), num_records * n), dtype=_edf_out_dtype("edf_decode", out_dtype))


_define("edf_decode", "(Tensor payload, int num_records, int R, int n, int[] chan_off, float[] gain, float[] offset, ScalarType? out_dtype=None) -> Tensor",
        _edf_decode_impl, _edf_decode_fake)


# ---- occlusion maps on the device (interpret.py: occlusion_maps) -------------------------------------------------------------------
OCCLUDE_MAX_LAYERS = 4       # EEG_OCCLUDE_MAX_LAYERS
OCCLUDE_MAX_GROUPS = 64       # EEG_OCCLUDE_MAX_GROUPS


def _aligned16(what, **tensors):
    for name, t in tensors.items():
        if t.data_ptr() % 16 != 0:
            raise RuntimeError(f"{what}: {name} is not 16-byte aligned (a view with an odd element offset): pass a tensor of its own")


def _occlude_expand_impl(x, hext, groups, lengths, t0: int, w: int, fill: float, x_var, h0_var, len_var) -> None:
    lib = _lib.get_lib()
    what = "occlude_expand"
    if not torch.is_tensor(x) or x.dim() != 4:
        raise RuntimeError(f"{what}: x must be (B, T, N, D) float32, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    _check(lib, x, "x")
    b, t, n, d = (int(v) for v in x.shape)
    dev = x.device
    layers = len(hext)
    if not 1 <= layers <= OCCLUDE_MAX_LAYERS:
        raise RuntimeError(f"{what}: {layers} layers (1..{OCCLUDE_MAX_LAYERS}: EEG_OCCLUDE_MAX_LAYERS)")
    if d < 4 or d % 4 != 0:
        raise RuntimeError(f"{what}: D={d}: the rows move in 16-byte pieces, D must be a positive multiple of 4")
    if not torch.is_tensor(groups) or groups.dim() != 2 or groups.shape[1] != n or not 1 <= groups.shape[0] <= OCCLUDE_MAX_GROUPS:
        raise RuntimeError(f"{what}: groups must be a (G, {n}) int32 0/1 mask with 1 <= G <= {OCCLUDE_MAX_GROUPS}, got "
                           f"{tuple(groups.shape) if torch.is_tensor(groups) else type(groups).__name__}")
    g = int(groups.shape[0])
    _eval_tensor(what, "groups", groups, torch.int32, (g, n), dev)
    if not 0 <= t0 < t or w < 1:
        raise RuntimeError(f"{what}: a window of w={w} steps at t0={t0} of T={t}")
    if hext[0].dim() != 3 or hext[0].shape[2] % n != 0:
        raise RuntimeError(f"{what}: hext must be (T+1, B, N*H), got {tuple(hext[0].shape)}")
    nh = int(hext[0].shape[2])
    if nh % 4 != 0:
        raise RuntimeError(f"{what}: N*H={nh} must be a multiple of 4")
    for layer, he in enumerate(hext):
        _eval_tensor(what, f"hext[{layer}]", he, torch.float32, (t + 1, b, nh), dev)
    if lengths is not None:
        _eval_tensor(what, "lengths", lengths, torch.int64, (b,), dev)
    _eval_tensor(what, "x_var", x_var, torch.float32, (t - t0, b * g, n, d), dev)
    _eval_tensor(what, "h0_var", h0_var, torch.float32, (layers, b * g, nh), dev)
    _eval_tensor(what, "len_var", len_var, torch.int64, (b * g,), dev)
    _aligned16(what, x=x, x_var=x_var, h0_var=h0_var, **{f"hext[{i}]": he for i, he in enumerate(hext)})
    tab = (ctypes.c_void_p * layers)(*[he.data_ptr() for he in hext])
    lib.call("eeg_dcrnn_occlude_expand", _p(x), tab, layers, _p(groups), _p(lengths), b, t, n, d, nh // n, g, int(t0), int(w), float(fill),
             _p(x_var), _p(h0_var), _p(len_var), _stream(x))


def _occlusion_scores_impl(var_logits, base_logits, lengths, target, k: int, t0: int, maps, base_prob, target_out) -> None:
    lib = _lib.get_lib()
    what = "occlusion_scores"
    if not torch.is_tensor(maps) or maps.dim() != 3 or min(maps.shape) < 1:
        raise RuntimeError(f"{what}: maps must be (B, Tw, G) float32, got {tuple(maps.shape) if torch.is_tensor(maps) else type(maps).__name__}")
    _check(lib, maps, "maps")
    b, tw, g = (int(v) for v in maps.shape)
    dev = maps.device
    if not torch.is_tensor(base_logits) or base_logits.dim() != 2 or base_logits.shape[0] != b or base_logits.shape[1] < 1:
        raise RuntimeError(f"{what}: base_logits must be ({b}, C) for maps {tuple(maps.shape)}, got "
                           f"{tuple(base_logits.shape) if torch.is_tensor(base_logits) else type(base_logits).__name__}")
    c = int(base_logits.shape[1])
    if g > OCCLUDE_MAX_GROUPS:
        raise RuntimeError(f"{what}: G={g} groups (1..{OCCLUDE_MAX_GROUPS}: EEG_OCCLUDE_MAX_GROUPS)")
    _eval_tensor(what, "base_logits", base_logits, torch.float32, (b, c), dev)
    _eval_tensor(what, "var_logits", var_logits, torch.float32, (b * g, c), dev)
    _eval_tensor(what, "base_prob", base_prob, torch.float32, (b,), dev)
    for name, t in (("lengths", lengths), ("target", target), ("target_out", target_out)):
        if t is not None:
            _eval_tensor(what, name, t, torch.int64, (b,), dev)
    if not 0 <= k < tw or t0 < 0:
        raise RuntimeError(f"{what}: window k={k} of Tw={tw} at t0={t0}")
    lib.call("eeg_dcrnn_occlusion_scores", _p(var_logits), _p(base_logits), _p(lengths), _p(target), b, g, c, tw, int(k), int(t0), _p(maps),
             _p(base_prob), _p(target_out), _stream(maps))


_define("occlude_expand", "(Tensor x, Tensor[] hext, Tensor groups, Tensor? lengths, int t0, int w, float fill, Tensor(a!) x_var, Tensor(b!) h0_var, "
        "Tensor(c!) len_var) -> ()", _occlude_expand_impl, lambda *a: None)
_define("occlusion_scores", "(Tensor var_logits, Tensor base_logits, Tensor? lengths, Tensor? target, int k, int t0, Tensor(a!) maps, "
        "Tensor(b!) base_prob, Tensor(c!)? target_out) -> ()", _occlusion_scores_impl, lambda *a: None)


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.n_in = len(inputs)


def _loss_backward(ctx, dloss, _dgrad):
    (dx,) = ctx.saved_tensors
    return (dx * dloss,) + (None,) * (ctx.n_in - 1)


for _name in ("bce_logits", "ce_logits", "masked_loss", "bce_logits_w", "ce_logits_w", "masked_loss_w", "bce_logits_cw", "ce_logits_cw"):
    torch.library.register_autograd(f"{NS}::{_name}", _loss_backward, setup_context=_loss_setup, lib=_libdef)


def _clip_adam_impl(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, beta1: float, beta2: float, eps: float,
                    weight_decay: float, max_norm: float, grad_scale: float, ws, norm_out):
    lib = _lib.get_lib()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _check(lib, t, nm)
    lib.call("eeg_dcrnn_clip_adam", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), params.numel(), float(max_norm),
             float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale),
             _p(ws), _p(norm_out), _stream(params))


_define("clip_adam_",
        "(Tensor(a!) params, Tensor(b!) grads, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, int step, float lr, float beta1, float beta2, "
        "float eps, float weight_decay, float max_norm, float grad_scale, Tensor(e!) ws, Tensor(f!)? norm_out) -> ()",
        _clip_adam_impl, lambda *a: None)


def _clip_adam_dev_impl(params, grads, exp_avg, exp_avg_sq, step_dev, lr_dev, beta1: float, beta2: float, eps: float,
                        weight_decay: float, max_norm: float, grad_scale: float, ws, norm_out):
    lib = _lib.get_lib()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (lr_dev, "lr_dev")):
        _check(lib, t, nm)
    _check(lib, step_dev, "step_dev", torch.int32)
    lib.call("eeg_dcrnn_clip_adam_dev", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), params.numel(), float(max_norm),
             _p(lr_dev), float(beta1), float(beta2), float(eps), float(weight_decay), _p(step_dev), float(grad_scale),
             _p(ws), _p(norm_out), _stream(params))


_define("clip_adam_dev_",
        "(Tensor(a!) params, Tensor(b!) grads, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, Tensor(g!) step_dev, Tensor lr_dev, float beta1, "
        "float beta2, float eps, float weight_decay, float max_norm, float grad_scale, Tensor(e!) ws, Tensor(f!)? norm_out) -> ()",
        _clip_adam_dev_impl, lambda *a: None)


def _teacher_flags_impl(rng_state, samples_seen, increment: int, cl_decay_steps: float, t_len: int):
    lib = _lib.get_lib()
    _check_rng(lib, rng_state, "rng_state")
    _check(lib, samples_seen, "samples_seen", torch.int64)
    flags = _new((t_len,), rng_state, torch.int32)
    lib.call("eeg_dcrnn_teacher_flags", _p(rng_state), _p(samples_seen), int(increment), float(cl_decay_steps), int(t_len),
             _p(flags), _stream(rng_state))
    return flags


_define("teacher_flags_", "(Tensor(a!) rng_state, Tensor(b!) samples_seen, int increment, float cl_decay_steps, int t_len) -> Tensor",
        _teacher_flags_impl, lambda rng_state, samples_seen, increment, cl_decay_steps, t_len: rng_state.new_empty((t_len,), dtype=torch.int32))


def _teacher_flags_dev_impl(rng_state, samples_seen, increment, cl_decay_steps: float, t_len: int):
    """`_teacher_flags_impl` with the increment read on the device: `increment` is one int64 on the device of the counter"""
    lib = _lib.get_lib()
    _check_rng(lib, rng_state, "rng_state")
    _check(lib, samples_seen, "samples_seen", torch.int64)
    if increment.dtype != torch.int64 or increment.numel() != 1 or increment.device != samples_seen.device:
        raise RuntimeError(f"teacher_flags: increment must be an int or one int64 on {samples_seen.device} (read on the device), got "
                           f"{increment.dtype} {tuple(increment.shape)} on {increment.device}")
    flags = _new((t_len,), rng_state, torch.int32)
    lib.call("eeg_dcrnn_teacher_flags_dev", _p(rng_state), _p(samples_seen), _p(increment.contiguous()), float(cl_decay_steps), int(t_len),
             _p(flags), _stream(rng_state))
    return flags


_define("teacher_flags_dev_", "(Tensor(a!) rng_state, Tensor(b!) samples_seen, Tensor increment, float cl_decay_steps, int t_len) -> Tensor",
        _teacher_flags_dev_impl, lambda rng_state, samples_seen, increment, cl_decay_steps, t_len: rng_state.new_empty((t_len,), dtype=torch.int32))


def _augment_draw_impl(rng_state, batch: int, swap_perm, plain_supports, reflected_supports):
    lib = _lib.get_lib()
    _check_rng(lib, rng_state, "rng_state")
    _check(lib, swap_perm, "swap_perm", torch.int32)
    n = swap_perm.numel()
    if batch < 1 or n < 1:
        raise RuntimeError(f"augment_draw: batch={batch}, num_nodes={n}")
    used = _rng_take_impl(rng_state, int(batch))
    flags = _new((batch,), rng_state, torch.int32)
    perm = _new((batch, n), rng_state, torch.int32)
    log_scale = _new((batch,), rng_state, torch.float32)
    nsup, s_out = 0, _new((0,), rng_state, torch.float32)
    if plain_supports is not None or reflected_supports is not None:
        if plain_supports is None or reflected_supports is None:
            raise RuntimeError("augment_draw: the per-clip supports need BOTH the plain and the reflected set")
        plain_supports, reflected_supports = plain_supports.contiguous(), reflected_supports.contiguous()
        _check(lib, plain_supports, "plain_supports")
        _check(lib, reflected_supports, "reflected_supports")
        if plain_supports.dim() != 3 or tuple(plain_supports.shape[1:]) != (n, n) or plain_supports.shape != reflected_supports.shape:
            raise RuntimeError(f"augment_draw: supports must be two (n_supports, {n}, {n}) tensors, got {tuple(plain_supports.shape)} and "
                               f"{tuple(reflected_supports.shape)}")
        nsup = plain_supports.shape[0]
        s_out = _new((nsup, batch, n, n), rng_state, torch.float32)
    lib.call("eeg_dcrnn_augment_draw", _p(used), int(batch), int(n), _p(swap_perm), _p(flags), _p(perm), _p(log_scale),
             _p(plain_supports) if nsup else None, _p(reflected_supports) if nsup else None, int(nsup), _p(s_out) if nsup else None,
             _stream(rng_state))
    return flags, perm, log_scale, s_out


def _augment_draw_fake(rng_state, batch, swap_perm, plain_supports, reflected_supports):
    n = swap_perm.numel()
    so = (0,) if plain_supports is None else (plain_supports.shape[0], batch, n, n)
    return (rng_state.new_empty((batch,), dtype=torch.int32), rng_state.new_empty((batch, n), dtype=torch.int32),
            rng_state.new_empty((batch,), dtype=torch.float32), rng_state.new_empty(so, dtype=torch.float32))


_define("augment_draw_", "(Tensor(a!) rng_state, int batch, Tensor swap_perm, Tensor? plain_supports, Tensor? reflected_supports) -> "
        "(Tensor, Tensor, Tensor, Tensor)", _augment_draw_impl, _augment_draw_fake)


# ---- epochs from a device-resident data set (the DataLoader's shuffle and collate, csrc/kernels_data.h) ----------------------------
def _epoch_keys_impl(keys, seed: int, epoch: int) -> None:
    """keys[i] <- the 63-bit Philox key of (seed, epoch, i): the epoch's permutation is their stable argsort"""
    lib = _lib.get_lib()
    _check(lib, keys, "keys", torch.int64)
    if keys.dim() != 1 or keys.numel() < 1:
        raise RuntimeError(f"epoch_keys: keys must be a non-empty int64 vector (one key per clip), got {tuple(keys.shape)}")
    if not 0 <= int(seed) < 2 ** 63 or not 0 <= int(epoch) < 2 ** 31:
        raise RuntimeError(f"epoch_keys: seed={seed} (0..2^63-1) / epoch={epoch} (0..2^31-1) out of range")
    lib.call("eeg_dcrnn_epoch_keys", int(seed), int(epoch), keys.numel(), _p(keys), _stream(keys))


_define("epoch_keys", "(Tensor(a!) keys, int seed, int epoch) -> ()", _epoch_keys_impl, lambda keys, seed, epoch: None)


def _gather_pair(lib, pool, out, name, dtypes, wide, dev):
    """one pool and its batch tensor -> (clips in the pool, bytes per clip); (0, 0) when absent"""
    if pool is None and out is None:
        return 0, 0
    if pool is None or out is None:
        raise RuntimeError(f"gather_clips: {name}_pool and {name}_out come together (one of them is None)")
    if pool.dtype not in dtypes:
        raise RuntimeError(f"gather_clips: {name}_pool must be {' or '.join(str(d) for d in dtypes)}, got {pool.dtype}")
    _check(lib, pool, f"{name}_pool", pool.dtype)
    _check(lib, out, f"{name}_out", pool.dtype)
    if pool.device != dev or out.device != dev:
        raise RuntimeError(f"gather_clips: {name}_pool is on {pool.device} and {name}_out on {out.device}, perm on {dev}: one device")
    if pool.dim() < 1 or out.dim() != pool.dim() or tuple(out.shape[1:]) != tuple(pool.shape[1:]) or pool.shape[0] < 1 or out.shape[0] < 1:
        raise RuntimeError(f"gather_clips: {name}_out {tuple(out.shape)} is not a batch of the clips of {name}_pool {tuple(pool.shape)}")
    if (pool.dim() > 1) != wide:
        raise RuntimeError(f"gather_clips: {name}_pool {tuple(pool.shape)} must be " + ("(P, ...): one row per clip" if wide else "(P,): one value per clip"))
    row = pool[0].numel() * pool.element_size()
    if wide and (row == 0 or row % 16 != 0):
        raise RuntimeError(f"gather_clips: a clip of {name}_pool has {row} bytes; the rows of a wide pool must be whole 16-byte pieces "
                           f"(a multiple of 4 floats per clip)")
    return pool.shape[0], row


def _gather_clips_impl(x_pool, x_out, y_pool, y_out, label_pool, label_out, len_pool, len_out, perm, cursor, rank: int, world: int,
                       clip_w=None, denom=None, n_valid=None) -> None:
    """x_out[b] <- x_pool[src_b] (and the second wide tensor, the labels, the lengths), src_b = clamp(perm[(cursor + rank*B + b) mod
    len(perm)], 0, P-1); cursor += B*world on the stream.  clip_w / denom / n_valid (the operator gather_clips_tail): the validity
    of the slots, written in front of the cursor's advance (eeg_dcrnn_gather_clips_tail)."""
    lib = _lib.get_lib()
    _check(lib, perm, "perm", torch.int64)
    _check(lib, cursor, "cursor", torch.int64)
    dev = perm.device
    if perm.dim() != 1 or perm.numel() < 1 or cursor.numel() != 1 or cursor.device != dev:
        raise RuntimeError(f"gather_clips: perm must be an int64 vector and cursor one int64 on its device, got {tuple(perm.shape)} / "
                           f"{tuple(cursor.shape)} on {cursor.device}")
    p, x_row = _gather_pair(lib, x_pool, x_out, "x", (torch.float32,), True, dev)
    b = x_out.shape[0]
    py, y_row = _gather_pair(lib, y_pool, y_out, "y", (torch.float32,), True, dev)
    pl, l_row = _gather_pair(lib, label_pool, label_out, "label", (torch.float32, torch.int64), False, dev)
    pn, _ = _gather_pair(lib, len_pool, len_out, "len", (torch.int64,), False, dev)
    for name, cnt, o in (("y", py, y_out), ("label", pl, label_out), ("len", pn, len_out)):
        if o is not None and (cnt != p or o.shape[0] != b):
            raise RuntimeError(f"gather_clips: {name}_pool holds {cnt} clips and {name}_out {o.shape[0]}; x_pool holds {p} and x_out {b}")
    if world < 1 or not 0 <= rank < world:
        raise RuntimeError(f"gather_clips: rank={rank} of world={world}")
    if b * world > perm.numel():
        raise RuntimeError(f"gather_clips: batch_size*world = {b * world} clips per step exceed the {perm.numel()} entries of perm")
    if clip_w is None:
        lib.call("eeg_dcrnn_gather_clips", _p(x_pool), _p(x_out), x_row, _p(y_pool), _p(y_out), y_row, _p(label_pool), _p(label_out), int(l_row),
                 _p(len_pool), _p(len_out), _p(perm), perm.numel(), int(p), _p(cursor), int(b), int(rank), int(world), _stream(perm))
        return
    for t, name, dtype, shape in ((clip_w, "clip_w", torch.float32, (b,)), (denom, "denom", torch.float32, (1,)), (n_valid, "n_valid", torch.int64, (1,))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"gather_clips: {name} must be a contiguous {dtype} tensor of shape {shape} on {dev} (written on the device), "
                               f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    lib.call("eeg_dcrnn_gather_clips_tail", _p(x_pool), _p(x_out), x_row, _p(y_pool), _p(y_out), y_row, _p(label_pool), _p(label_out), int(l_row),
             _p(len_pool), _p(len_out), _p(perm), perm.numel(), int(p), _p(cursor), int(b), int(rank), int(world), _p(clip_w), _p(denom),
             _p(n_valid), _stream(perm))


_define("gather_clips", "(Tensor x_pool, Tensor(a!) x_out, Tensor? y_pool, Tensor(b!)? y_out, Tensor? label_pool, Tensor(c!)? label_out, "
        "Tensor? len_pool, Tensor(d!)? len_out, Tensor perm, Tensor(e!) cursor, int rank, int world) -> ()", _gather_clips_impl, lambda *a: None)
_define("gather_clips_tail", "(Tensor x_pool, Tensor(a!) x_out, Tensor? y_pool, Tensor(b!)? y_out, Tensor? label_pool, Tensor(c!)? label_out, "
        "Tensor? len_pool, Tensor(d!)? len_out, Tensor perm, Tensor(e!) cursor, int rank, int world, Tensor(f!) clip_w, Tensor(g!) denom, "
        "Tensor(h!) n_valid) -> ()", _gather_clips_impl, lambda *a: None)


# ---- clips cut out of device-resident recordings (csrc/kernels_records.h) ----------------------------------------------------------
def _gather_records_impl(signals, rec_table, clip_table, label_pool, label_out, perm, cursor, rank: int, world: int, window: int, x_out,
                         y_out, len_out, clip_w=None, denom=None, n_valid=None) -> None:
    """x_out[b, n, :] <- the clip clip_table[src_b] = (rec, x_start, x_samples, y_start) of channel n of recording rec, cut out of
    `signals` through rec_table[rec] = (offset, stride, samples): whole steps of `window` samples, zeros behind them and outside the
    recording; y_out the same from y_start; len_out[b] the whole steps; src_b and the cursor as in gather_clips
    (eeg_dcrnn_gather_records)."""
    lib = _lib.get_lib()
    _check(lib, perm, "perm", torch.int64)
    _check(lib, cursor, "cursor", torch.int64)
    dev = perm.device
    if perm.dim() != 1 or perm.numel() < 1 or cursor.numel() != 1 or cursor.device != dev:
        raise RuntimeError(f"gather_records: perm must be an int64 vector and cursor one int64 on its device, got {tuple(perm.shape)} / "
                           f"{tuple(cursor.shape)} on {cursor.device}")
    _check(lib, signals, "signals", torch.float32)
    _check(lib, rec_table, "rec_table", torch.int64)
    _check(lib, clip_table, "clip_table", torch.int64)
    _check(lib, x_out, "x_out", torch.float32)
    given = [("signals", signals), ("rec_table", rec_table), ("clip_table", clip_table), ("x_out", x_out)]
    if y_out is not None:
        _check(lib, y_out, "y_out", torch.float32)
        given.append(("y_out", y_out))
    if len_out is not None:
        _check(lib, len_out, "len_out", torch.int64)
        given.append(("len_out", len_out))
    if (label_pool is None) != (label_out is None):
        raise RuntimeError("gather_records: label_pool and label_out come together (one of them is None)")
    if label_pool is not None:
        if label_pool.dtype not in (torch.float32, torch.int64):
            raise RuntimeError(f"gather_records: label_pool must be torch.float32 or torch.int64, got {label_pool.dtype}")
        _check(lib, label_pool, "label_pool", label_pool.dtype)
        _check(lib, label_out, "label_out", label_pool.dtype)
        given += [("label_pool", label_pool), ("label_out", label_out)]
    for name, t in given:
        if t.device != dev:
            raise RuntimeError(f"gather_records: {name} is on {t.device}, perm on {dev}: one device")
    if signals.dim() != 1 or signals.numel() < 4 or signals.numel() % 4 != 0:
        raise RuntimeError(f"gather_records: signals must be a flat float32 buffer of whole 16-byte pieces, got {tuple(signals.shape)}")
    if rec_table.dim() != 2 or rec_table.shape[0] < 1 or rec_table.shape[1] != 3:
        raise RuntimeError(f"gather_records: rec_table must be int64 (R, 3) = (offset, stride, samples), got {tuple(rec_table.shape)}")
    if clip_table.dim() != 2 or clip_table.shape[0] < 1 or clip_table.shape[1] != 4:
        raise RuntimeError(f"gather_records: clip_table must be int64 (P, 4) = (rec, x_start, x_samples, y_start), got {tuple(clip_table.shape)}")
    p = clip_table.shape[0]
    window = int(window)
    if window < 4 or window % 4 != 0:
        raise RuntimeError(f"gather_records: window={window} must be a positive multiple of 4 (rows of whole 16-byte pieces)")
    if x_out.dim() != 3 or x_out.numel() == 0 or x_out.shape[2] % window != 0:
        raise RuntimeError(f"gather_records: x_out must be (B, N, Tx*window) with window={window}, got {tuple(x_out.shape)}")
    b, n, x_len = x_out.shape
    y_len = 0
    if y_out is not None:
        if y_out.dim() != 3 or tuple(y_out.shape[:2]) != (b, n) or y_out.shape[2] == 0 or y_out.shape[2] % window != 0:
            raise RuntimeError(f"gather_records: y_out must be ({b}, {n}, Ty*window) with window={window}, got {tuple(y_out.shape)}")
        y_len = y_out.shape[2]
    if label_pool is not None and (tuple(label_pool.shape) != (p,) or tuple(label_out.shape) != (b,)):
        raise RuntimeError(f"gather_records: label_pool {tuple(label_pool.shape)} / label_out {tuple(label_out.shape)} must be ({p},) / ({b},): "
                           f"one value per clip of the table and of the batch")
    if len_out is not None and tuple(len_out.shape) != (b,):
        raise RuntimeError(f"gather_records: len_out must be int64 ({b},), got {tuple(len_out.shape)}")
    for name, t in (("x_out", x_out), ("y_out", y_out), ("signals", signals)):
        if t is not None and t.data_ptr() % 16 != 0:
            raise RuntimeError(f"gather_records: {name} at address {t.data_ptr():#x} is not 16-byte aligned")
    if world < 1 or not 0 <= rank < world:
        raise RuntimeError(f"gather_records: rank={rank} of world={world}")
    if b * world > perm.numel():
        raise RuntimeError(f"gather_records: batch_size*world = {b * world} clips per step exceed the {perm.numel()} entries of perm")
    if clip_w is not None:
        for t, name, dtype, shape in ((clip_w, "clip_w", torch.float32, (b,)), (denom, "denom", torch.float32, (1,)), (n_valid, "n_valid", torch.int64, (1,))):
            if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise RuntimeError(f"gather_records: {name} must be a contiguous {dtype} tensor of shape {shape} on {dev} (written on the device), "
                                   f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    lib.call("eeg_dcrnn_gather_records", _p(signals), signals.numel(), _p(rec_table), rec_table.shape[0], _p(clip_table), int(p), _p(label_pool),
             _p(label_out), 0 if label_pool is None else label_pool.element_size(), _p(perm), perm.numel(), _p(cursor), int(b), int(rank),
             int(world), int(n), window, int(x_len), int(y_len), _p(x_out), _p(y_out), _p(len_out), _p(clip_w), _p(denom), _p(n_valid),
             _stream(perm))


_define("gather_records", "(Tensor signals, Tensor rec_table, Tensor clip_table, Tensor? label_pool, Tensor(a!)? label_out, Tensor perm, "
        "Tensor(b!) cursor, int rank, int world, int window, Tensor(c!) x_out, Tensor(d!)? y_out, Tensor(e!)? len_out) -> ()",
        _gather_records_impl, lambda *a: None)
_define("gather_records_tail", "(Tensor signals, Tensor rec_table, Tensor clip_table, Tensor? label_pool, Tensor(a!)? label_out, Tensor perm, "
        "Tensor(b!) cursor, int rank, int world, int window, Tensor(c!) x_out, Tensor(d!)? y_out, Tensor(e!)? len_out, Tensor(f!) clip_w, "
        "Tensor(g!) denom, Tensor(h!) n_valid) -> ()", _gather_records_impl, lambda *a: None)


# =============================================================================================
# Python conveniences used by model/, utils.py and train_step.py
# =============================================================================================
# diagnostics: how often a layer took its input hop planes from the recurrent kernel of the layer below / ran its hoisted x-part
# in the eigenbasis of a shared symmetric support
hop_plane_handovers = 0
spectral_layer_calls = 0


def hop_polys(supports: Sequence[torch.Tensor], max_diffusion_step: int, batch: int) -> Tuple[torch.Tensor, int]:
    """Hop-polynomial matrices of the clip graphs (cell.py:83-93 incl. quirk Q1).

    supports: list of (N,N) or (B,N,N) tensors (torch.matmul broadcast semantics of cell.py:85).
    Returns (P (G, M-1, N, N), p_batched) with G = B if any support is batched else 1."""
    sups = list(supports)
    if len(sups) == 0:
        raise RuntimeError("hop_polys: empty supports list")
    flag = 1 if any(s.dim() == 3 for s in sups) else 0
    if flag or any(s.requires_grad for s in sups):
        return torch.ops.eeg_dcrnn.hop_polys(sups, int(max_diffusion_step), int(batch)), flag
    # graphs shared by all clips (2-D supports: the distance graph, one constant tensor for a whole run): the polynomials are a pure
    # function of the supports -- built once per supports tensors (identity + version), not once per forward
    import weakref
    key = (int(max_diffusion_step),) + tuple((s.data_ptr(), s._version, str(s.device), tuple(s.shape), s.dtype) for s in sups)
    hit = _polys_cache.get(key)
    if hit is not None and all(r() is s for r, s in zip(hit[0], sups)):
        return hit[1], 0
    out = torch.ops.eeg_dcrnn.hop_polys(sups, int(max_diffusion_step), int(batch))
    if not (out.is_cuda and torch.cuda.is_current_stream_capturing()):      # (a tensor born inside a capture lives in the graph's pool)
        if len(_polys_cache) > 64:
            for k in [k for k, v in _polys_cache.items() if any(r() is None for r in v[0])]:
                del _polys_cache[k]
        _polys_cache[key] = ([weakref.ref(s) for s in sups], out)
    return out, 0


# (max_diffusion_step, identity + version of every support) -> (weakrefs, P): see hop_polys
_polys_cache = {}


# id of a batched supports tensor -> (weakref, its 2-D form or None)
_shared_cache = {}


def collapse_shared_supports(supports):
    """[S (B,N,N)] whose B clips all carry the SAME graph -> [S[0] (N,N)]: the 2-D form declares the graph shared, which is what
    lets the encoder run the spectral form (`shared_spectral_basis`).  The reference's trainers always pass batched supports, even
    for the one distance graph, so `TrainStep` asks here.  Anything else (several supports, per-clip graphs, already
    2-D, spectral mode off) is returned unchanged.  The comparison reads one flag back from the device -- once per supports
    tensor (cached on its identity and version); under stream capture an unseen tensor is returned unchanged."""
    if not SPECTRAL_MODE or supports is None or len(supports) != 1 or not torch.is_tensor(supports[0]) or supports[0].dim() != 3:
        return supports
    import weakref
    sup = supports[0]
    key = (sup.data_ptr(), sup._version, str(sup.device), tuple(sup.shape), sup.dtype)
    hit = _shared_cache.get(key)
    if hit is not None and hit[0]() is sup:
        return supports if hit[1] is None else [hit[1]]
    if sup.is_cuda and torch.cuda.is_current_stream_capturing():
        return supports
    if len(_shared_cache) > 64:
        for k in [k for k, v in _shared_cache.items() if v[0]() is None]:
            del _shared_cache[k]
    same = sup.shape[0] >= 1 and bool((sup == sup[0:1]).all().item())
    flat = sup[0].to(torch.float32).clone() if same else None
    _shared_cache[key] = (weakref.ref(sup), flat)
    return supports if flat is None else [flat]


def fft_features(raw: torch.Tensor, window: int = 200, mean: Optional[float] = None, std: Optional[float] = None,
                 perm: Optional[torch.Tensor] = None, log_scale: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
                 padding_val: float = 0.0):
    """Input featurisation on the device: raw (B,N,T*window) resampled signals ->
    (feat_raw (B,T,N,window/2) log|FFT| per 1-s step, feat_std = the standardised (and optionally
    augmented) model input or None when mean/std are not given).

    Replaces `computeFFT` per step (data_utils.py:13-35, dataloader_detection.py:57-71), the reflection /
    amplitude-jitter augmentation (perm (B,N) int32 source channel per node, log_scale (B);
    dataloader_detection.py:233-256) and `StandardScaler.transform` (utils.py:393-428).

    lengths (B,) int64 on the device of `raw`: variable-length clips (dataloader_classification.py:25-85,321-343: the short clip is
    augmented and standardised, then padded with `padding_val`).  Clip b has clamp(lengths[b], 1, T) valid windows; the windows
    behind them are not transformed -- feat_std holds `padding_val` there and feat_raw 0 -- and the valid ones are bit-identical
    to the call without lengths.  The kernel reads the lengths: no host synchronisation, a captured call replays with new ones."""
    std_on = mean is not None
    if lengths is not None:
        _clip_lengths("fft_features", lengths, raw.shape[0], raw)
        fr, fs = torch.ops.eeg_dcrnn.fft_features_len(raw, int(window), float(mean) if std_on else 0.0, float(std) if std is not None else 1.0,
                                                      std_on, perm, log_scale, lengths, float(padding_val))
        return fr, (fs if std_on else None)
    fr, fs = torch.ops.eeg_dcrnn.fft_features(raw, int(window), float(mean) if std_on else 0.0,
                                              float(std) if std is not None else 1.0, std_on, perm, log_scale)
    return fr, (fs if std_on else None)


def fft_features_pair(raw_x: torch.Tensor, raw_y: torch.Tensor, window: int = 200, mean: float = 0.0, std: float = 1.0,
                      perm: Optional[torch.Tensor] = None, log_scale: Optional[torch.Tensor] = None):
    """Featurisation of an SSL sample, which is a pair: raw_x (B,N,Tx*window) input and raw_y (B,N,Ty*window) target signals ->
    (feat_raw_x (B,Tx,N,window/2): log|FFT| of the un-augmented input, the operand of the correlation graph;
     x_std (B,Tx,N,window/2), y_std (B,Ty,N,window/2): both halves reflected by the clip's `perm[b]`, shifted by the clip's
     `log_scale[b]` and standardised with (mean, std)).

    Replaces dataloader_ssl.py:317-341 on top of `computeFFT` per step: one coin and one scale factor per sample, applied to the
    input AND the target, then the scaler on both.  window = 200: one launch for the pair, every output bit-identical to
    `fft_features` on that half; another window: the general kernel once per half.  Forward-only: the inputs of a training
    step carry no gradient."""
    return torch.ops.eeg_dcrnn.fft_features_pair(raw_x, raw_y, int(window), float(mean), float(std), perm, log_scale)


def window_features(raw: torch.Tensor, window: int, mean: float, std: float, perm: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None, padding_val: float = 0.0):
    """Time-domain input of the model on the device (the reference without --use_fft): raw (B,N,T*window) resampled signals ->
    (B,T,N,window) = (raw[b, perm[b][n], t*window ..] * scale[b] - mean) / std: the windowing of `computeSliceMatrix(is_fft=False)`
    (dataloader_detection.py:25-85), `_random_reflect` / `_random_scale` (`EEG_seq *= scale_factor`, :233-256) and
    `StandardScaler.transform` (utils.py:393-428) in one pass.  perm (B,N) int32 source channel per node, scale (B) the clip's
    amplitude factor; None = no reflection / factor 1.  Forward-only.
    lengths (B,) int64 on the device of `raw` (dataloader_classification.py:25-85,321-343): the steps t >= clamp(lengths[b], 1, T) of
    clip b are not read and hold `padding_val`; every other value is bit-identical to the call without lengths."""
    if lengths is not None:
        _clip_lengths("window_features", lengths, raw.shape[0], raw)
        return torch.ops.eeg_dcrnn.window_features_len(raw, int(window), float(mean), float(std), perm, scale, lengths, float(padding_val))
    return torch.ops.eeg_dcrnn.window_features(raw, int(window), float(mean), float(std), perm, scale)


def window_features_pair(raw_x: torch.Tensor, raw_y: torch.Tensor, window: int, mean: float, std: float,
                         perm: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """`window_features` of an SSL pair in one launch (dataloader_ssl.py:159-182,317-341: one coin and one factor per sample on
    input AND target, the scaler on both): raw_x (B,N,Tx*window), raw_y (B,N,Ty*window) -> (x_std (B,Tx,N,window), y_std
    (B,Ty,N,window)), each bit-identical to `window_features` on that half."""
    return torch.ops.eeg_dcrnn.window_features_pair(raw_x, raw_y, int(window), float(mean), float(std), perm, scale)


def augment_windows(x: torch.Tensor, y: Optional[torch.Tensor], perm: torch.Tensor, scale: torch.Tensor, mean: float, std: float):
    """The time-domain augmentation on already STANDARDISED windows, one launch for x (B,Tx,N,D) and an optional y (B,Ty,N,D):
    out[b, t, n] = in[b, t, perm[b][n]] * scale[b] + (scale[b] - 1) * mean / std -- multiplying the signals by s in front of the
    scaler (mean, std) = this behind it.  D a multiple of 4; perm (B,N) int32, scale (B).  Returns (x_aug, y_aug or None), new
    tensors.  Forward-only."""
    xa, ya = torch.ops.eeg_dcrnn.augment_windows(x, y, perm, scale, float(mean), float(std))
    return xa, (ya if y is not None else None)


def augment_features(x: torch.Tensor, y: torch.Tensor, perm: torch.Tensor, log_scale: torch.Tensor, feature_std: float):
    """The reflection / amplitude-jitter augmentation of an SSL pair of already STANDARDISED features, one launch:
    x_aug[b, t, n] = x[b, t, perm[b][n]] + log_scale[b] / feature_std, and the same for y (each with its own number of steps).
    x (B,Tx,N,D), y (B,Ty,N,D), D a multiple of 4; perm (B,N) int32 source channel per node, log_scale (B) = log of the clip's
    amplitude factor, feature_std = the StandardScaler's std (dataloader_ssl.py:159-182,317-341: the reference adds log(factor)
    BEFORE it standardises).  Returns (x_aug, y_aug), new tensors.  Forward-only: the inputs of a training step carry no gradient."""
    return torch.ops.eeg_dcrnn.augment_features(x, y, perm, log_scale, float(feature_std))


def correlation_supports(x: torch.Tensor, top_k: int = 3, return_adj: bool = False, lengths: Optional[torch.Tensor] = None):
    """Per-clip correlation graph -> [S1, S2] dual random-walk supports, on the device.

    x (B,T,N,D) clips (the model input); D <= 128 (features) runs the kernel that stages whole time steps, a wider D (time-domain
    windows, D = 200) the kernel for wide channel rows.  Replaces the DataLoader-side `_get_indiv_graphs` +
    `keep_topk` + `_compute_supports('dual_random_walk')` (dataloader_detection.py:258-307,335-354).
    lengths (B,) int64 on the device of x: the graph of the UNPADDED clips (dataloader_classification.py:356-361) -- only the steps
    t < clamp(lengths[b], 1, T) of clip b enter it, whatever the padded steps hold.
    Returns [S1 (B,N,N), S2 (B,N,N)] (and the sparsified adjacency (B,N,N) if return_adj)."""
    wide = x.dim() == 4 and x.shape[3] > 128
    if lengths is not None:
        _clip_lengths("correlation_supports", lengths, x.shape[0], x)
        adj, s1, s2 = (torch.ops.eeg_dcrnn.corr_graph_rows_len(x, int(top_k), lengths, int(x.shape[1])) if wide
                       else torch.ops.eeg_dcrnn.corr_graph_len(x, int(top_k), lengths))
        return ([s1, s2], adj) if return_adj else [s1, s2]
    adj, s1, s2 = (torch.ops.eeg_dcrnn.corr_graph_rows if wide else torch.ops.eeg_dcrnn.corr_graph)(x, int(top_k))
    return ([s1, s2], adj) if return_adj else [s1, s2]


def correlation_supports_raw(raw: torch.Tensor, top_k: int = 3, return_adj: bool = False, lengths: Optional[torch.Tensor] = None,
                             window: int = 200):
    """The same graph for a time-domain clip, from its raw signals: raw (B,N,L) channel rows, L a multiple of 4 (the clip of
    `computeSliceMatrix(is_fft=False)` reshaped by `_get_indiv_graphs` to (N, T*200) is these rows again; dataloader_detection.py:
    25-85,258-307).  Returns [S1 (B,N,N), S2 (B,N,N)] (and the sparsified adjacency if return_adj).
    lengths (B,) int64 on the device of raw: clips of L / window steps of `window` samples (a multiple of 4) of which clip b has
    clamp(lengths[b], 1, L / window) -- the graph of its first lengths[b] * window samples per row (dataloader_classification.py:
    356-361: the unpadded clip); `window` is read only then."""
    if raw.dim() != 3:
        raise RuntimeError(f"raw signals must be (B, N, L) channel rows, got {tuple(raw.shape)}")
    if lengths is not None:
        if window < 4 or window % 4 != 0 or raw.shape[2] % window != 0 or raw.shape[2] == 0:
            raise RuntimeError(f"correlation_supports_raw: rows of {raw.shape[2]} samples are not whole steps of window={window} samples "
                               f"(a positive multiple of 4)")
        _clip_lengths("correlation_supports_raw", lengths, raw.shape[0], raw)
        adj, s1, s2 = torch.ops.eeg_dcrnn.corr_graph_rows_len(raw, int(top_k), lengths, int(raw.shape[2] // window))
        return ([s1, s2], adj) if return_adj else [s1, s2]
    adj, s1, s2 = torch.ops.eeg_dcrnn.corr_graph_rows(raw, int(top_k))
    return ([s1, s2], adj) if return_adj else [s1, s2]


def pack_cell(wg, bg, wc, bc, fin: int, h: int, m: int) -> torch.Tensor:
    """Reference-layout cell parameters -> MFMA-fragment-ordered device block (kernels_pack.h)."""
    return torch.ops.eeg_dcrnn.pack_cell(wg, bg, wc, bc, fin, h, m)


def diffusion_hops(x: torch.Tensor, p: torch.Tensor, p_batched: int, batch: int) -> torch.Tensor:
    """The diffusion step alone: x (S,N,F) -> (M-1,S,N,F) hop planes P_m x (micro-benchmark entry;
    north_star's HBM-bound kernel)."""
    return torch.ops.eeg_dcrnn.diffusion_hops(x, p, int(p_batched), int(batch))


def dconv(x, p, p_batched, weight, biases):
    """DiffusionGraphConv.forward (cell.py:66-118) on x (B,N,F): HIP diffusion + fp32-MFMA GEMM with
    the reference-layout weight ((F*M), O); differentiable w.r.t. x, weight and biases."""
    return torch.ops.eeg_dcrnn.dconv(x, p, int(p_batched), weight, biases)


class LayerOut:
    """what one layer hands on: hext (T+1,B,N*H) with hseq = hext[1:], hsel (B,N*H) and — when the backward
    pass will run — the hop planes hpl (M-1,T+1,B,N,H) whose slots 1..T are the next layer's input planes"""
    __slots__ = ("hext", "hsel", "hpl")

    def __init__(self, hext, hsel, hpl):
        self.hext, self.hsel, self.hpl = hext, hsel, hpl

    @property
    def hseq(self):
        return self.hext[1:]


def pack_encoder_cells(cells, basis, num_nodes):
    """(packs, spacks) of the cells of an encoder from ONE launch (`pack_cells`), or None where the cells pack themselves (a single
    layer, more than four, the opt-in bf16 split).  spacks is a list of None without a basis."""
    cells = list(cells)
    if len(cells) < 2 or len(cells) > 4 or GEMM_MODE != 0:
        return None
    h, m = cells[0]._num_units, cells[0].num_matrices
    if basis is not None and h != 64:
        basis = None
    # (detached: the packs are a re-layout the layer operators consume next to the parameters themselves, whose gradients come from
    #  the layer operators' backward)
    out = torch.ops.eeg_dcrnn.pack_cells([c.dconv_gate.weight.detach() for c in cells], [c.dconv_gate.biases.detach() for c in cells],
                                         [c.dconv_candidate.weight.detach() for c in cells], [c.dconv_candidate.biases.detach() for c in cells],
                                         h, m, basis, int(num_nodes))
    k = len(cells)
    return out[:k], (out[k:] if basis is not None else [None] * k)


def dcgru_layer_ex(x, x_off, h0, p, p_batched, wg, bg, wc, bc, n, h, m, activation="tanh", lengths=None, x_planes=None,
                   want_hsel=True, basis=None, pack=None, spack=None) -> LayerOut:
    """One DCGRU layer over x (T + x_off, B, N, Fin).  x_off = 1 / x_planes: x is the `hext` of the layer below and
    x_planes its `hpl` (the layer then skips its own diffusion pass).  want_hsel=False: the caller does not read the layer's
    final state (hsel comes back empty; saves one copy per step).  basis (`shared_spectral_basis`): the hoisted x-part of the
    layer runs in the eigenbasis of the shared symmetric support where the kernels cover the shape (else the general path)."""
    act = ACT_CODES.get(activation, 1)
    save = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, h0, wg, bg, wc, bc))
    if basis is not None:
        need_dx = 1 if (save and x.requires_grad) else 0
        dims = _layer_dims(x.shape[0] - x_off, x.shape[1], n, h, x.shape[3], m, act, int(p_batched), False)
        if p_batched or not _lib.get_lib().query("eeg_dcrnn_spectral_ok", ctypes.byref(dims), need_dx):
            basis = None
        else:
            if x_planes is not None and x_planes.dim() != 3:
                x_planes = None            # (hop planes of a layer that took the general path)
            global spectral_layer_calls
            spectral_layer_calls += 1
    if basis is None and x_planes is not None and x_planes.dim() != 5:
        x_planes = None                    # (the U^T h of a spectral layer is of no use to the general path)
    if x_planes is not None:
        global hop_plane_handovers
        hop_plane_handovers += 1
    hext, hsel, saved = torch.ops.eeg_dcrnn.dcgru_layer(x, int(x_off), h0, p, int(p_batched), wg, bg, wc, bc, lengths, x_planes,
                                                        n, h, m, act, save, bool(want_hsel), basis, pack,
                                                        spack if basis is not None else None)
    return LayerOut(hext, hsel, saved[7].detach() if (save and saved[7].numel()) else None)


# (data_ptr, version, device, shape) of a support tensor -> (weakref to it, basis or None): the eigenbasis is a pure function of the
# support, the distance graph is one constant tensor for a whole run, and its residual has to be READ once (a device-to-host
# synchronisation) to know that the support is symmetric -- neither belongs into a training step.
_basis_cache = {}


def shared_spectral_basis(supports, max_diffusion_step: int):
    """The eigenbasis block of the support when the spectral form applies: exactly ONE support, given as a 2-D (N,N) tensor
    (= declared shared by all clips; batched supports always take the general path), at least one diffusion step, and
    |S - U diag(lam) U^T| at rounding level (S symmetric: filter_type "laplacian" on an undirected graph).  Else None.
    The first call for a support synchronises once to read the residual; under stream capture an unseen support gets None."""
    if not SPECTRAL_MODE or max_diffusion_step < 1 or len(supports) != 1:
        return None
    sup = supports[0]
    if sup.dim() != 2 or sup.shape[0] != sup.shape[1] or sup.shape[0] < 2 or sup.shape[0] > 32:
        return None
    import weakref
    key = (sup.data_ptr(), sup._version, str(sup.device), tuple(sup.shape), sup.dtype)
    hit = _basis_cache.get(key)
    if hit is not None and hit[0]() is sup:
        return hit[1]
    if sup.is_cuda and torch.cuda.is_current_stream_capturing():
        return None
    if len(_basis_cache) > 64:
        for k in [k for k, v in _basis_cache.items() if v[0]() is None]:
            del _basis_cache[k]
    basis = torch.ops.eeg_dcrnn.spectral_basis(sup)
    n = sup.shape[0]
    info = basis[n * n + 256:n * n + 259].tolist()        # residual, off-diagonal left, max |S|  (one synchronisation per support)
    ok = info[0] <= SPECTRAL_TOL * max(info[2], 1e-30) and info[1] <= 1e-9 * max(info[2], 1e-30)
    _basis_cache[key] = (weakref.ref(sup), basis if ok else None)
    return basis if ok else None


def dcgru_layer(x, h0, p, p_batched, wg, bg, wc, bc, n, h, m, activation="tanh", lengths=None):
    """Run one DCGRU layer over x (T,B,N,Fin).  Returns (hseq (T,B,N*H), hsel (B,N*H))."""
    out = dcgru_layer_ex(x, 0, h0, p, p_batched, wg, bg, wc, bc, n, h, m, activation, lengths)
    return out.hseq, out.hsel


def dcgru_decoder(targets, h0, p, p_batched, first_cell, shared_cell, wp, bp, n, h, dout, m, n_layers,
                  activation="tanh", teacher=None, dropout_p=0.0, rng_state=None, return_rng_used=False):
    """Run the whole decoder: returns (T,B,N*Dout).  first_cell / shared_cell = (wg, bg, wc, bc).  dropout_p > 0: nn.Dropout
    in front of the projection, masks from the device generator rng_state (make_rng_state; advanced in place)."""
    act = ACT_CODES.get(activation, 1)
    t_len = targets.shape[0]
    sc = shared_cell if shared_cell is not None else (None, None, None, None)
    # teacher: a sequence of T host flags, or a DEVICE int32[T] tensor (ops.teacher_flags: drawn on the stream, graph-replayable)
    tf_dev = teacher if torch.is_tensor(teacher) else None
    use_tf = tf_dev is not None or (teacher is not None and any(teacher))
    tf = [1 if v else 0 for v in teacher] if (use_tf and tf_dev is None) else [0] * t_len     # never an empty list: pytree leaf of the autograd glue
    used = rng_take(rng_state, t_len * h0.shape[1] * n * h // 4) if dropout_p > 0 else None
    out, _ = torch.ops.eeg_dcrnn.dcgru_decoder(targets if use_tf else None, h0, p, int(p_batched), *first_cell, *sc, wp, bp, tf,
                                               int(t_len), n, h, dout, m, n_layers, act, float(dropout_p), used, tf_dev)
    return (out, used) if return_rng_used else out


def cls_head(z, w, bias, dropout_p=0.0, rng_state=None, return_rng_used=False):
    """model.py:267-270: dropout (training) -> relu -> per-node Linear(H->C) -> max over nodes, one launch; the dropout mask
    comes from the device generator rng_state (make_rng_state) and is recomputed, not stored, in the backward."""
    used = rng_take(rng_state, z.numel() // 4) if dropout_p > 0 else None
    logits, _ = torch.ops.eeg_dcrnn.cls_head(z, w, bias, float(dropout_p), used)
    return (logits, used) if return_rng_used else logits


def _weights_together(what, clip_w, denom, ref, clip_u=None):
    """the pair of the weighted criteria: both or none, and on the device of the clips (the dispatcher picks the implementation by
    the devices of ALL tensor arguments: a stray one is refused here, by name; dtype and shape are the operator's to refuse).
    clip_u (the multipliers of `clip_weights`) takes the place of clip_w (the selector of the validity gather): never both."""
    if clip_u is not None:
        if clip_w is not None:
            raise RuntimeError(f"{what}: clip_w (which clips count) and clip_u (a multiplier per clip; 0 selects a clip out) are mutually "
                               f"exclusive: fold the validity into clip_u (ops.clip_weights does)")
        if denom is None:
            raise RuntimeError(f"{what}: clip_u and denom come together (denom is None)")
        _clip_weights(what, clip_u, denom, clip_u.numel() if torch.is_tensor(clip_u) and clip_u.dim() == 1 else -1, ref, "clip_u")
        return
    if (clip_w is None) != (denom is None):
        raise RuntimeError(f"{what}: clip_w and denom come together (one of them is None)")
    if clip_w is not None:
        _clip_weights(what, clip_w, denom, clip_w.numel() if torch.is_tensor(clip_w) and clip_w.dim() == 1 else -1, ref)


def cls_head_loss(z, fc_weight, fc_bias, targets, task="detection", dropout_p=0.0, rng_state=None, clip_w=None, denom=None, clip_u=None):
    """The tail of a supervised optimisation step behind the encoder (model.py:267-270 + train.py:203-206,266-272) in two launches:
    dropout -> relu -> fc -> max over nodes, the criterion (task "detection": BCE-with-logits, "classification": cross-entropy) and
    their backward.  z (B,N,H) = the top layer's state at len-1, DETACHED from autograd: the gradients of fc go straight into
    `fc_weight.grad` / `fc_bias.grad` (written in place inside `with GradSink`, else accumulated), and the caller seeds the encoder's
    backward with the returned dz (`last.backward(dz)`).  Returns (loss (), logits (B,C), dz (B,N,H)).
    clip_w (B,) float32 / denom (1,) float32, both on the device and given together (`gather_clips(..., clip_w=, denom=, n_valid=)`,
    an epoch's short last batch): the mean runs over the clips with clip_w != 0 and divides by denom; the others get dz = 0 and add
    nothing to the loss and to the gradients of fc, whatever their label holds.  logits are returned for every clip.
    clip_u (B,) float32 >= 0 with denom, instead of clip_w (`clip_weights`: class / sample weights): loss = sum_b u_b * l_b / denom and
    every gradient carries u_b / denom; u_b == 0 selects the clip out as clip_w == 0 does."""
    _weights_together("cls_head_loss", clip_w, denom, z, clip_u)
    used = rng_take(rng_state, z.numel() // 4) if dropout_p > 0 else None
    sunk = [GradSink.take(q) for q in (fc_weight, fc_bias)]
    dw = sunk[0] if sunk[0] is not None else _new_like(fc_weight)
    db = sunk[1] if sunk[1] is not None else _new_like(fc_bias)
    kind = 0 if task == "detection" else 1
    if clip_u is not None:
        loss, logits, _arg, _dl, dz = torch.ops.eeg_dcrnn.cls_head_loss_cw(z.detach(), fc_weight.detach(), fc_bias.detach(), targets,
                                                                           kind, float(dropout_p), used, clip_u, denom, dw, db)
    elif clip_w is None:
        loss, logits, _arg, _dl, dz = torch.ops.eeg_dcrnn.cls_head_loss(z.detach(), fc_weight.detach(), fc_bias.detach(), targets,
                                                                        kind, float(dropout_p), used, dw, db)
    else:
        loss, logits, _arg, _dl, dz = torch.ops.eeg_dcrnn.cls_head_loss_w(z.detach(), fc_weight.detach(), fc_bias.detach(), targets,
                                                                          kind, float(dropout_p), used, clip_w, denom, dw, db)
    for q, buf, sk in ((fc_weight, dw, sunk[0]), (fc_bias, db, sunk[1])):
        if sk is None and q.requires_grad:
            q.grad = buf if q.grad is None else q.grad + buf
    return loss[0], logits, dz


def rng_take(rng_state, groups):
    """hand out the generator's current {seed, offset} pair for `groups` Philox counters and advance the device state"""
    if rng_state is None:
        raise RuntimeError("dropout_p > 0 needs a device generator state (ops.make_rng_state)")
    return torch.ops.eeg_dcrnn.rng_take_(rng_state, int(groups))


def dropout_mask(rng_used, n, dropout_p):
    """the keep-mask x 1/(1-p) factors of elements 0..n-1 for a forward call's {seed, offset} pair (tests)"""
    return torch.ops.eeg_dcrnn.dropout_mask(rng_used, int(n), float(dropout_p))


def gather_last(htop: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """utils.last_relevant_pytorch on a time-major (T,B,D) tensor, no host sync (forward only)."""
    return torch.ops.eeg_dcrnn.gather_last(htop, lengths)


def masked_regression_loss(y_predicted, y_true, mean=None, std=None, loss_fn="mae", mask_val=0.0, clip_w=None, denom=None):
    """utils.compute_regression_loss (utils.py:431-495).  Only the exact string 'mae' selects the MAE
    (utils.py:489-495); anything else is the masked RMSE.
    clip_w (B,) / denom (1,) (float32 on the device, together; B = the leading dimension): the loss L over the elements of the clips
    with clip_w != 0 only, times the rank's factor sum(clip_w) / denom -- on one rank with denom = the number of such clips, L itself."""
    _weights_together("masked_regression_loss", clip_w, denom, y_predicted)
    scaled = mean is not None
    args = (y_predicted, y_true, scaled, float(mean) if scaled else 0.0, float(std) if scaled else 1.0, float(mask_val), 0 if loss_fn == "mae" else 1)
    if clip_w is None:
        return torch.ops.eeg_dcrnn.masked_loss(*args)[0]
    return torch.ops.eeg_dcrnn.masked_loss_w(*args, clip_w, denom)[0]


def bce_with_logits(logits, y, clip_w=None, denom=None, clip_u=None):
    """nn.BCEWithLogitsLoss() (mean): value and dlogits from one HIP launch (train.py:203-204).
    clip_w (B,) / denom (1,) (float32 on the device, together): sum over the clips with clip_w != 0, divided by denom.
    clip_u (B,) >= 0 with denom, instead of clip_w: sum_b u_b * l_b / denom -- u_b = y_b ? p : 1, denom = B is `pos_weight=p` on 0 / 1
    labels (`clip_weights(class_w=(1, p), norm="count")`)."""
    _weights_together("bce_with_logits", clip_w, denom, logits, clip_u)
    if clip_u is not None:
        return torch.ops.eeg_dcrnn.bce_logits_cw(logits, y, clip_u, denom)[0]
    if clip_w is None:
        return torch.ops.eeg_dcrnn.bce_logits(logits, y)[0]
    return torch.ops.eeg_dcrnn.bce_logits_w(logits, y, clip_w, denom)[0]


def cross_entropy(logits, y, clip_w=None, denom=None, clip_u=None):
    """nn.CrossEntropyLoss() (mean) on (B,C) logits and int64 class targets (train.py:205-206).
    clip_w (B,) / denom (1,) (float32 on the device, together): sum over the clips with clip_w != 0, divided by denom; the label of
    a clip that does not count is not looked at.
    clip_u (B,) >= 0 with denom, instead of clip_w: sum_b u_b * l_b / denom -- u_b = w[y_b], denom = sum_b u_b is `weight=w`
    (`clip_weights(class_w=w, norm="sum")`)."""
    _weights_together("cross_entropy", clip_w, denom, logits, clip_u)
    if clip_u is not None:
        return torch.ops.eeg_dcrnn.ce_logits_cw(logits, y, clip_u, denom)[0]
    if clip_w is None:
        return torch.ops.eeg_dcrnn.ce_logits(logits, y)[0]
    return torch.ops.eeg_dcrnn.ce_logits_w(logits, y, clip_w, denom)[0]


def decoder_is_persistent(t_len, batch, n, h, dout, m, n_layers) -> bool:
    """the persistent decoder kernels cover this shape (then device-resident teacher-forcing flags are available)"""
    lib = _lib.get_lib()
    dims = _dec_dims((int(t_len), int(batch), int(n), int(h), int(dout), int(m), int(n_layers), 0, 0))
    return bool(lib.query("eeg_dcrnn_decoder_is_persistent", ctypes.byref(dims)))


def teacher_flags(rng_state, samples_seen, increment, cl_decay_steps, t_len):
    """Scheduled-sampling flags of one decoder forward drawn ON THE DEVICE (model.py:194-200, utils.py:385-390): int32[t_len],
    flag t = u_t < k / (k + exp(samples_seen / k)); advances the generator and adds `increment` to samples_seen on the stream.
    increment: an int, or one int64 ON THE DEVICE that is read on the stream (`n_valid` of `gather_clips`: the real size of an
    epoch's short last batch inside a replayed graph)."""
    if torch.is_tensor(increment):
        return torch.ops.eeg_dcrnn.teacher_flags_dev_(rng_state, samples_seen, increment, float(cl_decay_steps), int(t_len))
    return torch.ops.eeg_dcrnn.teacher_flags_(rng_state, samples_seen, int(increment), float(cl_decay_steps), int(t_len))


def draw_augmentation(rng_state, batch, swap_perm, plain_supports=None, reflected_supports=None):
    """The reference's per-sample augmentation draws (dataloader_detection.py:233-256,384-389), ON THE DEVICE from a Philox
    generator state (`make_rng_state`; advanced on the stream: a captured step draws afresh at every replay): per clip a fair coin
    -- reflect along the midline or not -- and a scale factor uniform in [0.8, 1.2).
    swap_perm: int32 (N,) source channel of every node of a reflected clip (`utils.swap_permutation`).
    plain_supports / reflected_supports: lists (or stacked tensors) of the (N,N) supports of the distance graph and of its reflected
    partner (`utils.compute_supports` / `utils.reflected_supports`); given, the per-clip supports are returned as well.
    Returns (flags int32 (B,), perm int32 (B,N), log_scale float32 (B,), supports: list of (B,N,N) tensors or None) -- `perm` and
    `log_scale` are the operands of `fft_features`."""
    stack = lambda t: None if t is None else (t if torch.is_tensor(t) else torch.stack(list(t)))   # noqa: E731
    ps, rs = stack(plain_supports), stack(reflected_supports)
    if ps is not None and ps.dim() == 2:
        ps, rs = ps[None], rs[None]
    flags, perm, log_scale, s_out = torch.ops.eeg_dcrnn.augment_draw_(rng_state, int(batch), swap_perm, ps, rs)
    return flags, perm, log_scale, (None if ps is None else [s_out[i] for i in range(s_out.shape[0])])


def clip_adam_step_dev(params, grads, exp_avg, exp_avg_sq, step_dev, lr_dev, betas, eps, weight_decay, max_norm, grad_scale, ws,
                       norm_out=None):
    """clip_adam_step with the step counter (int32[1], incremented on the stream) and the learning rate (float32[1]) in device
    memory: capturable into a HIP graph together with the rest of the step."""
    torch.ops.eeg_dcrnn.clip_adam_dev_(params, grads, exp_avg, exp_avg_sq, step_dev, lr_dev, float(betas[0]), float(betas[1]),
                                       float(eps), float(weight_decay), float(max_norm), float(grad_scale), ws, norm_out)


def clip_adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay, max_norm, grad_scale, ws,
                   norm_out=None):
    """Fused clip_grad_norm_ + Adam (coupled L2) over flat fp32 buffers (train.py:273-275)."""
    torch.ops.eeg_dcrnn.clip_adam_(params, grads, exp_avg, exp_avg_sq, int(step), float(lr), float(betas[0]), float(betas[1]),
                                   float(eps), float(weight_decay), float(max_norm), float(grad_scale), ws, norm_out)


def clip_weights(labels, clip_u, denom, class_w=None, sample_w=None, norm="sum", perm=None, cursor=None, back: int = 0, rank: int = 0, world: int = 1):
    """The multipliers of one step's criterion and their divisor, written on the device into clip_u (B,) float32 and denom (1,) float32
    (fixed addresses, one launch, capturable): u = valid * class_w[class(label)] * sample_w[src], every factor optional.  class(label):
    the int64 label (outside 0..C-1: weight 1), or label >= 0.5 for detection's float labels, which are taken to be 0 or 1 (class_w
    has two entries then).  norm "sum": denom = sum of u over the step / world (`nn.CrossEntropyLoss(weight=)`; a zero sum gives 1);
    "count": denom = max(n_valid, 1) / world (`nn.BCEWithLogitsLoss(pos_weight=p)` with class_w = (1, p)).
    Batch form (perm=None): labels (B,) are the batch's own, every slot is valid, the divisor is the rank's own (world is ignored:
    data-parallel, the result is the mean of the ranks' weighted means); no sample_w.
    Sampler form (perm=, cursor= of an `EpochSampler`): labels is the label pool (P,), sample_w (P,) goes with it, and the kernel
    walks all batch_size*world slots of the step through perm from the cursor as the step's gather saw it -- back=0 in front of the
    gather, back=batch_size*world behind it -- with the validity rule of a drop_last=False epoch: every rank gets its own slice of
    the weights and the same global divisor / world, with no communication."""
    if norm not in WEIGHT_NORMS:
        raise RuntimeError(f"clip_weights: norm={norm!r} ('sum' or 'count')")
    for name, t in (("labels", labels), ("clip_u", clip_u), ("denom", denom)):
        if not torch.is_tensor(t):
            raise RuntimeError(f"clip_weights: {name} must be a tensor, got {type(t).__name__}")
    for name, t in (("clip_u", clip_u), ("denom", denom), ("class_w", class_w), ("sample_w", sample_w), ("perm", perm), ("cursor", cursor)):
        if t is not None and (not torch.is_tensor(t) or t.device != labels.device):      # (the dispatcher would route a stray tensor by its key)
            raise RuntimeError(f"clip_weights: {name} must be a tensor on {labels.device} (the labels' device), got "
                               f"{t.device if torch.is_tensor(t) else type(t).__name__}")
    torch.ops.eeg_dcrnn.clip_weights(labels, perm, cursor, int(back), int(rank), int(world), class_w, sample_w, WEIGHT_NORMS[norm], clip_u, denom)
    return clip_u, denom


def epoch_keys(keys: torch.Tensor, seed: int, epoch: int) -> torch.Tensor:
    """the shuffle keys of epoch `epoch` under `seed`, written into `keys` (int64 (P,)); `torch.sort(keys, stable=True)` gives the
    epoch's permutation (the DataLoader's RandomSampler, dataloader_detection.py:505-523) -- `device_data.EpochSampler.begin_epoch`"""
    torch.ops.eeg_dcrnn.epoch_keys(keys, int(seed), int(epoch))
    return keys


def gather_clips(x_pool, x_out, perm, cursor, rank: int = 0, world: int = 1, y_pool=None, y_out=None, label_pool=None, label_out=None,
                 len_pool=None, len_out=None, clip_w=None, denom=None, n_valid=None):
    """One step's batch out of the device-resident pools (the DataLoader's collate): slot b of the batch tensors takes clip
    clamp(perm[(cursor + rank*B + b) mod len(perm)], 0, P-1) of every pool given -- x (wide), y (a second wide tensor: the SSL
    target), a float / int64 label and an int64 length per clip -- and `cursor` (int64[1], on the device) advances by B*world on the
    stream.  Two launches, no allocation, capturable.
    clip_w (B,) float32, denom (1,) float32, n_valid (1,) int64, on the device and given together: an epoch that keeps its short
    last batch.  The same copy -- the slots behind the end of the epoch hold real clips through the wrap -- and, written in front of
    the cursor's advance: clip_w[b] = 1 if 0 <= cursor + rank*B + b < len(perm) else 0, n_valid = clamp(len(perm) - cursor, 0,
    B*world) (all ranks), denom = max(n_valid, 1) / world -- the operands of the weighted criteria (`cls_head_loss`, `bce_with_logits`,
    `cross_entropy`, `masked_regression_loss`) and of `teacher_flags`.  A full batch: clip_w = 1, denom = B."""
    tail = [t is not None for t in (clip_w, denom, n_valid)]
    if not any(tail):
        torch.ops.eeg_dcrnn.gather_clips(x_pool, x_out, y_pool, y_out, label_pool, label_out, len_pool, len_out, perm, cursor, int(rank), int(world))
        return
    if not all(tail):
        raise RuntimeError("gather_clips: clip_w, denom and n_valid come together (one of them is None)")
    torch.ops.eeg_dcrnn.gather_clips_tail(x_pool, x_out, y_pool, y_out, label_pool, label_out, len_pool, len_out, perm, cursor, int(rank),
                                          int(world), clip_w, denom, n_valid)


def gather_records(signals, rec_table, clip_table, x_out, perm, cursor, rank: int = 0, world: int = 1, *, window: int, y_out=None,
                   label_pool=None, label_out=None, len_out=None, clip_w=None, denom=None, n_valid=None):
    """One step's batch CUT out of device-resident recordings (the reference loaders' slicing at __getitem__ time): slot b takes clip
    src = clamp(perm[(cursor + rank*B + b) mod len(perm)], 0, P-1) of clip_table (P, 4) int64 = (rec, x_start, x_samples, y_start).
    signals: flat float32 buffer; rec_table (R, 3) int64 = (offset, stride, samples), sample s of channel n of recording r at
    offset + n*stride + s.  x_out (B, N, Tx*window): the whole steps of the x_samples from x_start on, exactly 0.0 behind them and
    outside the recording; y_out (B, N, Ty*window), optional: the same from y_start over its whole length; len_out (B,) int64,
    optional: the whole steps kept; label_out (B,) <- label_pool (P,).  `cursor` advances by B*world on the stream.  Two launches, no
    allocation, capturable.  clip_w / denom / n_valid: as in `gather_clips`.  No table entry makes the kernel read outside
    `signals` or write outside the batch tensors (`device_data.RecordingDataset` validates its table on the host all the same)."""
    tail = [t is not None for t in (clip_w, denom, n_valid)]
    if not any(tail):
        torch.ops.eeg_dcrnn.gather_records(signals, rec_table, clip_table, label_pool, label_out, perm, cursor, int(rank), int(world),
                                           int(window), x_out, y_out, len_out)
        return
    if not all(tail):
        raise RuntimeError("gather_records: clip_w, denom and n_valid come together (one of them is None)")
    torch.ops.eeg_dcrnn.gather_records_tail(signals, rec_table, clip_table, label_pool, label_out, perm, cursor, int(rank), int(world),
                                            int(window), x_out, y_out, len_out, clip_w, denom, n_valid)


def eval_scores(logits, label_pool, clip_w, cursor, probs, losses, rank: int = 0, world: int = 1):
    """Per-clip scores of one step of an evaluation pass over a pool in order, behind `gather_clips(..., clip_w=, denom=, n_valid=)`
    (which has advanced `cursor`): slot b of logits (B, C) is pool position cursor - B*world + rank*B + b; a slot with clip_w != 0
    and a position in [0, P) writes probs[pos] (sigmoid, C = 1 / the softmax row) and losses[pos] (the BCE-with-logits /
    cross-entropy term of that clip, label read from label_pool[pos]: float32 (P,) for C = 1, int64 (P,) else).  Nothing is ever
    written outside probs (P,) / (P, C) and losses (P,).  One launch, no allocation, capturable."""
    torch.ops.eeg_dcrnn.eval_scores(logits, label_pool, clip_w, cursor, int(rank), int(world), probs, losses)


def eval_metrics(probs, labels, losses, search: bool = False, thresh: float = 0.5, ws=None, record=None):
    """The scores of a pool from its per-clip scores, on the device, as one int64 record (include/eeg_dcrnn.h: eeg_dcrnn_eval_metrics;
    `evaluation.scores_from_record` turns it into the reference's score dictionary): detection (probs (P,), labels float32) -- the
    clips sorted by the project's own bitonic sort, AUROC numerator, the max-F1 threshold of `utils.thresh_max_f1` (search=True) or
    `thresh`, the confusion counts of prob > threshold; classification (probs (P, C), labels int64) -- the C x C confusion matrix of
    the first arg-max.  ws / record: `eval_metrics_buffers` (allocated here when not given).  Returns record; no host sync."""
    if ws is None or record is None:
        ws, record = eval_metrics_buffers(probs.shape[0], 1 if probs.dim() == 1 else probs.shape[1], probs.device)
    torch.ops.eeg_dcrnn.eval_metrics(probs, labels, losses, bool(search), float(thresh), ws, record)
    return record


def ssl_eval_scores(pred, target, clip_w, cursor, scores, rank: int = 0, world: int = 1, mean=None, std=None, mask_val: float = 0.0, keep=None):
    """Per-clip masked-MAE sums of one step of an SSL evaluation pass over a pool in order, behind `gather_clips(..., clip_w=, denom=,
    n_valid=)` (which has advanced `cursor`): slot b of pred / target (B, Ty, N, D) is pool position cursor - B*world + rank*B + b; a
    slot with clip_w != 0 and a position in [0, P) writes scores[:, pos] = (float64 sum of the float32 |d| over its masked-in
    elements, their number, the number of those whose d is not finite -- left out of the sum), with d and the mask as in
    `masked_regression_loss(..., mean, std, "mae", mask_val)`.  A clip's sum does not depend on B, the slot or the rank, bit for bit.
    keep (P, Ty, N, D): the slot's pred is copied to keep[pos].  Nothing is ever written outside scores (3, P) and keep.  One launch,
    no allocation, capturable."""
    scaled = mean is not None
    torch.ops.eeg_dcrnn.ssl_eval_scores(pred, target, clip_w, cursor, int(rank), int(world), scaled, float(mean) if scaled else 0.0,
                                        float(std) if scaled else 1.0, float(mask_val), scores, keep)


def ssl_eval_metrics(scores, group: int, record=None):
    """The record of an SSL evaluation pass from its (3, P) scores, on the device, as SSL_EVAL_RECORD_WORDS float64 words named by
    SSL_EVAL_RECORD: n, batches = ceil(P / group), loss = the reference's AverageMeter over consecutive batches of `group` clips (a
    batch with nothing masked in counts 0 with its weight), pool_mae = sum abs_sum / sum count (independent of group), the totals of
    abs_sum, count and bad, empty_batches.  record: `ssl_eval_buffers` (allocated here when not given).  Returns record; no host sync."""
    if record is None:
        record = torch.zeros(SSL_EVAL_RECORD_WORDS, dtype=torch.float64, device=scores.device)
    torch.ops.eeg_dcrnn.ssl_eval_metrics(scores, int(group), record)
    return record


def feature_moments(raw, scores, clip_w, cursor, rank: int = 0, world: int = 1, *, window: Optional[int] = None, use_fft: bool = True, lengths=None):
    """Per-clip moments of the UN-standardised model inputs of a gathered batch, one step of a scaler fit (`statistics.fit_scaler`).
    raw: raw signals (B, N, T*window) -- use_fft=True: the values are the float32 log|FFT| features `fft_features` returns as
    feat_raw for the batch, bit for bit and never stored (window % 4 == 0, at most 252; 200: the mixed-radix transform); use_fft=
    False: the samples themselves -- or ready features / windows (B, T, N, D) with window=None, always taken as given.  lengths:
    None or int64 (B,) on the device: clip b counts its first clamp(lengths[b], 1, T) steps only.  scores: (4, P) float64 (sum |
    sumsq | count | bad; `moments_buffers`): slot b is pool position cursor - B*world + rank*B + b and writes its four words there
    only if clip_w[b] != 0 and 0 <= position < P (clip_w None: every slot counts; cursor None: position rank*B + b).  A NaN or
    infinite value is counted in bad and left out of the sums.  No floating-point atomics; a clip's words have the same bits whatever
    B, slot, rank, cursor and length.  Operands that do not fit raise ValueError before any launch.  Returns scores; no host sync."""
    for name, t in (("raw", raw), ("lengths", lengths), ("clip_w", clip_w), ("cursor", cursor)):      # (the dispatcher would route a stray
        if torch.is_tensor(t) and torch.is_tensor(scores) and t.device != scores.device:               # device by its own rules)
            raise ValueError(f"feature_moments: {name} is on {t.device}, scores on {scores.device}: one device")
    torch.ops.eeg_dcrnn.feature_moments(raw, lengths, clip_w, cursor, int(rank), int(world), 0 if window is None else int(window), bool(use_fft),
                                        scores)
    return scores


def moments_record(scores, record=None):
    """The record of a scaler fit from its (4, P) scores, on the device, as MOMENTS_RECORD_WORDS float64 words named by
    MOMENTS_RECORD: clips (positions with count > 0), count, sum, sumsq, mean = sum / count, std = sqrt(sumsq / count - mean^2)
    (the population std, np.std), bad.  A variance at or below 2^-50 * sumsq lies inside the rounding of the sums (negative values
    among them) and gives std = 0: a pool of equal values reports 0, not noise.  count == 0: mean = std = 0.  One block, an order
    that depends on P alone.  record: `moments_buffers` (allocated here when not given).  Returns record; no host sync."""
    if record is None:
        record = torch.zeros(MOMENTS_RECORD_WORDS, dtype=torch.float64, device=scores.device if torch.is_tensor(scores) else None)
    torch.ops.eeg_dcrnn.moments_record(scores, record)
    return record


class ScanBuffers:
    """the tensors of one scan's post-processing (`scan_buffers`): bin_off (R + 1,) int64; timeline, smoothed (total_bins,) float32;
    cover (total_bins,) int32; events (R, E_max, 2) int32; event_count (R,) int32; record (SCAN_RECORD_WORDS,) and rec_records (R,
    SCAN_RECORD_WORDS) int64"""

    def __init__(self, rec_steps, max_events: int, device, zeroed: bool = True):
        steps = [int(v) for v in rec_steps]
        if not 1 <= len(steps) <= SCAN_MAX_RECORDINGS or min(steps) < 0:
            raise ValueError(f"scan_buffers: rec_steps names {len(steps)} recordings (1..{SCAN_MAX_RECORDINGS}) of >= 0 whole steps each")
        off = [0]
        for v in steps:
            off.append(off[-1] + v)
        if not 1 <= off[-1] < 1 << 31:
            raise ValueError(f"scan_buffers: the recordings hold {off[-1]} whole steps in all (1..2^31-1): nothing to scan")
        if int(max_events) < 1:
            raise ValueError(f"scan_buffers: max_events={max_events}: E_max < 1 holds no event")
        r, total = len(steps), off[-1]
        self.bin_off = torch.tensor(off, dtype=torch.int64, device=device)
        new = torch.zeros if zeroed else torch.empty                     # (the kernels write every element of every output)
        self.timeline = new(total, dtype=torch.float32, device=device)
        self.smoothed = new(total, dtype=torch.float32, device=device)
        self.cover = new(total, dtype=torch.int32, device=device)
        self.events = new((r, int(max_events), 2), dtype=torch.int32, device=device)
        self.event_count = new(r, dtype=torch.int32, device=device)
        self.record = new(SCAN_RECORD_WORDS, dtype=torch.int64, device=device)
        self.rec_records = new((r, SCAN_RECORD_WORDS), dtype=torch.int64, device=device)


def scan_buffers(rec_steps, max_events: int, device, zeroed: bool = True):
    """The buffers of `scan_timeline` / `scan_events` / `event_scores` for recordings of rec_steps[r] whole steps (bins) each and at
    most max_events events per recording, as a `ScanBuffers` (zeroed, or uninitialised: the kernels write every element); allocated
    once per result by the caller (`scan.Scanner`)"""
    return ScanBuffers(rec_steps, max_events, device, zeroed)


def _monotone(what, name, t, last=None):
    """host check (one small device-to-host copy) of an offset table: starts at 0, never decreases, ends at `last`"""
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 2:
        return None                                                      # (the operator refuses it by shape and dtype)
    v = t.cpu().tolist()
    if v[0] != 0 or any(b < a for a, b in zip(v, v[1:])) or (last is not None and v[-1] != last):
        raise ValueError(f"{what}: {name} is not a monotone offset table from 0" + ("" if last is None else f" to {last}") +
                         f" (first offending entries: {v[:8]})")
    return v


def scan_check_tables(clip_table, clip_off, bin_off, x_steps: int, window: int, num_clips=None, total_bins=None, what: str = "scan_timeline"):
    """Host validation of the tables of a scan (device-to-host copies: call it once per table, `Scanner` does): bin_off and clip_off
    monotone from 0 (to total_bins / P), and the rows of every recording name it, start at whole, strictly ascending steps and are all
    x_steps*window samples long -- what `clip_table_scan` builds.  Anything else raises ValueError."""
    _monotone(what, "bin_off", bin_off, total_bins)
    off = _monotone(what, "clip_off", clip_off, num_clips)
    if off is None or not torch.is_tensor(clip_table) or clip_table.dim() != 2 or clip_table.shape[1] != 4 or clip_table.dtype != torch.int64:
        return
    table = clip_table.cpu().numpy()
    if off[-1] != table.shape[0]:
        raise ValueError(f"{what}: clip_off ends at {off[-1]}, the table has {table.shape[0]} rows")
    for r in range(len(off) - 1):
        rows = table[off[r]:off[r + 1]]
        if not len(rows):
            continue
        if (rows[:, 0] != r).any():
            raise ValueError(f"{what}: rows {off[r]}..{off[r + 1]} of the table belong to recording {r} by clip_off and name another one")
        if (rows[:, 2] != x_steps * window).any():
            raise ValueError(f"{what}: the rows of recording {r} are not all x_steps*window = {x_steps * window} samples long (clip_table_scan)")
        if (rows[:, 1] < 0).any() or (rows[:, 1] % window != 0).any() or (np.diff(rows[:, 1]) <= 0).any():
            raise ValueError(f"{what}: the rows of recording {r} do not start at whole, ascending steps of {window} samples (clip_table_scan)")


def _same_device(what, anchor_name, anchor, **tensors):
    for name, t in tensors.items():
        if torch.is_tensor(t) and torch.is_tensor(anchor) and t.device != anchor.device:
            raise ValueError(f"{what}: {name} is on {t.device}, {anchor_name} on {anchor.device}: one device")


def scan_timeline(probs, clip_table, clip_off, bin_off, timeline, cover, *, x_steps: int, window: int, agg: str = "mean", validate: bool = True):
    """The per-bin probability timeline of whole recordings from the probabilities of their overlapping clips (one bin = one step of
    `window` samples).  probs (P,) float32, one per row of clip_table (P, 4) int64; recording r owns the rows clip_off[r] ..
    clip_off[r+1] and the bins bin_off[r] .. bin_off[r+1] (`clip_table_scan`, `scan_buffers`).  Bin j of a recording is covered by its
    rows with start_step <= j < start_step + x_steps -- found from the start steps in the table by binary search, a gather -- and
    gets agg="mean": the float32 sum of their probabilities in ascending row order over float(cover), or agg="max": their maximum;
    an uncovered bin gets 0 and cover 0.  Every element of timeline (total_bins,) float32 and cover (total_bins,) int32 is written.
    validate: check the tables on the host first (`scan_check_tables`; two small copies).  Returns (timeline, cover)."""
    if agg not in SCAN_AGG:
        raise ValueError(f"scan_timeline: agg={agg!r} (one of {sorted(SCAN_AGG)})")
    _same_device("scan_timeline", "timeline", timeline, probs=probs, clip_table=clip_table, clip_off=clip_off, bin_off=bin_off, cover=cover)
    if validate:
        scan_check_tables(clip_table, clip_off, bin_off, int(x_steps), int(window), probs.numel() if torch.is_tensor(probs) else None,
                          timeline.numel() if torch.is_tensor(timeline) else None)
    torch.ops.eeg_dcrnn.scan_timeline(probs, clip_table, clip_off, bin_off, int(x_steps), int(window), SCAN_AGG[agg], timeline, cover)
    return timeline, cover


def scan_thresholds(th_on, th_off=None):
    """(th_on, th_off) rounded to float32 ONCE, as Python floats: the values the kernel compares with (th_off None: th_on)"""
    on = float(th_on)
    off = on if th_off is None else float(th_off)
    if on != on or off != off:
        raise ValueError(f"scan_events: a threshold is NaN (th_on={th_on}, th_off={th_off})")
    if off > on:
        raise ValueError(f"scan_events: th_off={off} above th_on={on} (hysteresis: on at th_on, off below th_off <= th_on)")
    return float(np.float32(on)), float(np.float32(off))


def scan_events(timeline, cover, bin_off, smoothed, events, event_count, *, smooth_bins: int = 1, th_on: float = 0.5, th_off=None,
                merge_gap: int = 0, min_bins: int = 1, validate: bool = True):
    """Seizure events of every recording from its timeline, one workgroup per recording, bins streamed through LDS in chunks of
    SCAN_CHUNK_BINS.  Per recording: q_j = the float32 ascending sum of the timeline over the covered bins of [j-h, j+h] inside the
    recording over their number, h = (smooth_bins-1)/2 (odd, <= SCAN_MAX_SMOOTH_BINS; 0 for an uncovered j) -> smoothed; state_j on if
    q_j >= th_on, off if q_j < th_off or j is uncovered, else state_{j-1} (thresholds rounded to float32 once here); maximal runs of on
    are events [onset, offset); a run at most merge_gap off bins behind the event before it is merged into it (chains); events shorter
    than min_bins are then dropped.  events (R, E_max, 2) int32 in order with zero rows behind them, event_count (R,) int32 the TRUE
    number -- it may exceed E_max, the rows behind E_max are never written.  Returns (smoothed, events, event_count); no host sync
    with validate=False (validate: bin_off monotone, one small copy)."""
    on, off = scan_thresholds(th_on, th_off)
    _same_device("scan_events", "timeline", timeline, cover=cover, bin_off=bin_off, smoothed=smoothed, events=events, event_count=event_count)
    if validate:
        _monotone("scan_events", "bin_off", bin_off, timeline.numel() if torch.is_tensor(timeline) else None)
    torch.ops.eeg_dcrnn.scan_events(timeline, cover, bin_off, int(smooth_bins), on, off, int(merge_gap), int(min_bins), smoothed, events, event_count)
    return smoothed, events, event_count


def event_scores(events, event_count, ref, ref_count, cover, bin_off, record, rec_records, *, validate: bool = True):
    """Event- and bin-level scores of detected events against reference intervals (`annotation_bins`: ref (R, A_max, 2) int32 half-open
    bin intervals, ref_count (R,) int32) as int64 words named by SCAN_RECORD: per recording in rec_records (R, SCAN_RECORD_WORDS), summed
    in record: n_ref, n_hyp = min(event_count, E_max), ref_hit / hyp_hit (events of one side sharing a bin with one of the other),
    covered_bins, tp / fp / fn / tn over the covered bins, overflowed (recordings with event_count > E_max).  Returns record."""
    _same_device("event_scores", "cover", cover, events=events, event_count=event_count, ref=ref, ref_count=ref_count, bin_off=bin_off,
                 record=record, rec_records=rec_records)
    if validate:
        _monotone("event_scores", "bin_off", bin_off, cover.numel() if torch.is_tensor(cover) else None)
    torch.ops.eeg_dcrnn.event_scores(events, event_count, ref, ref_count, cover, bin_off, record, rec_records)
    return record


def occlude_expand(x, hext, groups, lengths, t0: int, w: int, fill: float, x_var, h0_var, len_var):
    """The B*G variants of ONE occlusion window (steps [t0, t0 + w)) of x (B, T, N, D), variant v = b*G + g, into buffers the caller
    owns: x_var (T - t0, B*G, N, D) time-major -- `fill` where the step lies inside the window and groups[g, n] != 0, else
    x[b, t0 + s, n, :] --, h0_var (L, B*G, N*H) = hext[l][t0, b] for every g (hext: the (T+1, B, N*H) state sequences of the encoder
    layers of the unoccluded pass, L <= OCCLUDE_MAX_LAYERS) and len_var (B*G,) int64 = max(lengths[b] - t0, 1) (lengths None: T - t0).
    groups: (G, N) int32 0/1 on the device, G <= OCCLUDE_MAX_GROUPS; an empty group occludes nothing.  A copy kernel: bit for bit, in
    16-byte pieces (D % 4 == 0, N*H % 4 == 0, 16-byte aligned tensors).  One launch, no allocation."""
    torch.ops.eeg_dcrnn.occlude_expand(x, list(hext), groups, lengths, int(t0), int(w), float(fill), x_var, h0_var, len_var)


def occlusion_scores(var_logits, base_logits, lengths, target, k: int, t0: int, maps, base_prob, target_out=None):
    """Slice k of an occlusion map from the logits of its window's variants: maps[b, k, g] = p_b - p_{b,k,g} with p = sigmoid(logit)
    (one output) or softmax(logits)[target_b]; exactly 0.0 where the window starts at or behind the clip's end (t0 >= lengths[b]).
    target: int64 (B,) on the device -- a class outside 0..C-1 is CLAMPED in the kernel -- or None: the arg-max of the baseline row,
    lowest index on ties.  The probabilities are evaluated in double from the float32 logits.  k == 0 also writes base_prob (B,) and
    (if given) the classes followed to target_out (B,) int64.  One launch, no allocation, no host synchronisation."""
    torch.ops.eeg_dcrnn.occlusion_scores(var_logits, base_logits, lengths, target, int(k), int(t0), maps, base_prob, target_out)


# ---- the clustered bootstrap of the scores on the device (bootstrap.py; csrc/kernels_boot.h) ---------------------------------------
BOOT_MAX_GROUPS = 1 << 20             # EEG_BOOT_MAX_GROUPS: clusters of one call
BOOT_MAX_REPLICATES = 65535           # EEG_BOOT_MAX_REPLICATES
BOOT_DET_WORDS = 10                   # EEG_BOOT_DET_WORDS: int64 words of a replicate's detection record
BOOT_MAX_CLASSES = 32                 # EEG_BOOT_MAX_CLASSES
BOOT_MAX_RECORD_WORDS = 64            # EEG_BOOT_MAX_RECORD_WORDS: K of boot_records
BOOT_LDS_GROUPS = 32768               # EEG_BOOT_LDS_GROUPS: the widest counts row a replicate's workgroup keeps in LDS
BOOT_RECORD = ("weight", "pos", "neg", "auroc_num", "tp", "fp", "fn", "tn", "ap_bits", "loss_bits")     # the words of a detection record


def _boot_counts_arg(what, lib, counts, g=None):
    """(n_boot, G, device) of a counts tensor (n_boot + 1, G) int32"""
    if not torch.is_tensor(counts) or counts.dim() != 2 or counts.dtype != torch.int32 or not counts.is_contiguous():
        got = f"{counts.dtype} {tuple(counts.shape)}" if torch.is_tensor(counts) else type(counts).__name__
        raise ValueError(f"{what}: counts must be a contiguous torch.int32 tensor of shape (n_boot + 1, G), got {got}")
    if lib.is_device_build and not counts.is_cuda:
        raise ValueError(f"{what}: the tensors are on {counts.device}; eeg_gnn_ssl_amd runs only on an MI355X (HIP) device and has no CPU path")
    n_boot, width = int(counts.shape[0]) - 1, int(counts.shape[1])
    if g is not None and width != g:
        raise ValueError(f"{what}: counts rows are {width} wide, the clips name G={g} clusters")
    if not 1 <= width <= BOOT_MAX_GROUPS:
        raise ValueError(f"{what}: G={width} clusters outside 1..{BOOT_MAX_GROUPS} (EEG_BOOT_MAX_GROUPS)")
    if not 1 <= n_boot <= BOOT_MAX_REPLICATES:
        raise ValueError(f"{what}: n_boot={n_boot} replicates outside 1..{BOOT_MAX_REPLICATES} (EEG_BOOT_MAX_REPLICATES)")
    return n_boot, width, counts.device


def _boot_counts_impl(seed: int, counts) -> None:
    lib = _lib.get_lib()
    n_boot, g, _ = _boot_counts_arg("boot_counts", lib, counts)
    if not 0 <= int(seed) < 1 << 63:
        raise ValueError(f"boot_counts: seed={seed} outside 0..2^63-1")
    lib.call("eeg_dcrnn_boot_counts", int(seed), g, n_boot, _p(counts), _stream(counts))


def _boot_pool(what, probs, groups, counts, max_cluster):
    """the checks the two clip-level operators share -> (lib, P, C, G, n_boot, device)"""
    lib = _lib.get_lib()
    if not torch.is_tensor(probs) or probs.dim() not in (1, 2) or probs.shape[0] < 1 or (probs.dim() == 2 and probs.shape[1] < 2):
        got = f"{tuple(probs.shape)}" if torch.is_tensor(probs) else type(probs).__name__
        raise ValueError(f"{what}: probs must be (P,) (detection) or (P, C) with C >= 2 (classification), got {got}")
    p, c = int(probs.shape[0]), (1 if probs.dim() == 1 else int(probs.shape[1]))
    if p > EVAL_MAX_CLIPS:
        raise ValueError(f"{what}: P={p} clips exceed the limit of one call, {EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    n_boot, g, dev = _boot_counts_arg(what, lib, counts, None if groups is not None else p)
    _scan_tensor(what, "probs", probs, torch.float32, (p,) if c == 1 else (p, c), dev)
    if groups is not None:
        _scan_tensor(what, "groups", groups, torch.int32, (p,), dev)
    if int(max_cluster) < 1 or g * int(max_cluster) >= 1 << 31:
        raise ValueError(f"{what}: G={g} clusters, the largest of {int(max_cluster)} clips: G * largest must stay below 2^31 (a replicate's weight "
                         f"fits 31 bits); use fewer, smaller clusters")
    return lib, p, c, g, n_boot, dev


def _boot_ws(what, lib, ws, p, dev):
    need = (int(lib.query("eeg_dcrnn_boot_ws_bytes", p)) + 7) // 8
    if not torch.is_tensor(ws) or ws.dtype != torch.int64 or ws.dim() != 1 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise ValueError(f"{what}: ws must be a contiguous int64 vector of at least {need} entries on {dev} (ops.boot_workspace)")


def _boot_detection_impl(probs, labels, groups, losses, counts, thresh: float, max_cluster: int, ws, records) -> None:
    what = "boot_detection"
    lib, p, c, g, n_boot, dev = _boot_pool(what, probs, groups, counts, max_cluster)
    if c != 1:
        raise ValueError(f"{what}: probs must be (P,), got {tuple(probs.shape)} (classification: ops.boot_classification)")
    _scan_tensor(what, "labels", labels, torch.float32, (p,), dev)
    if losses is not None:
        _scan_tensor(what, "losses", losses, torch.float32, (p,), dev)
    if thresh != thresh:
        raise ValueError(f"{what}: thresh is NaN")
    _boot_ws(what, lib, ws, p, dev)
    _scan_tensor(what, "records", records, torch.int64, (n_boot + 1, BOOT_DET_WORDS), dev)
    lib.call("eeg_dcrnn_boot_detection", _p(probs), _p(labels), _p(groups), _p(losses), p, g, int(max_cluster), _p(counts), n_boot, float(thresh),
             _p(ws), _p(records), _stream(probs))


def _boot_classification_impl(probs, labels, groups, counts, max_cluster: int, ws, records) -> None:
    what = "boot_classification"
    lib, p, c, g, n_boot, dev = _boot_pool(what, probs, groups, counts, max_cluster)
    if not 2 <= c <= BOOT_MAX_CLASSES:
        raise ValueError(f"{what}: probs must be (P, C) with 2 <= C <= {BOOT_MAX_CLASSES} (EEG_BOOT_MAX_CLASSES), got {tuple(probs.shape)}")
    _scan_tensor(what, "labels", labels, torch.int64, (p,), dev)
    _boot_ws(what, lib, ws, p, dev)
    _scan_tensor(what, "records", records, torch.int64, (n_boot + 1, c * c), dev)
    lib.call("eeg_dcrnn_boot_classification", _p(probs), _p(labels), _p(groups), p, c, g, int(max_cluster), _p(counts), n_boot, _p(ws), _p(records),
             _stream(probs))


def _boot_records_impl(rec_records, counts, records) -> None:
    what = "boot_records"
    lib = _lib.get_lib()
    n_boot, g, dev = _boot_counts_arg(what, lib, counts)
    if not torch.is_tensor(rec_records) or rec_records.dim() != 2 or not 1 <= rec_records.shape[1] <= BOOT_MAX_RECORD_WORDS:
        got = f"{tuple(rec_records.shape)}" if torch.is_tensor(rec_records) else type(rec_records).__name__
        raise ValueError(f"{what}: rec_records must be (G, K) int64 with 1 <= K <= {BOOT_MAX_RECORD_WORDS} (EEG_BOOT_MAX_RECORD_WORDS), got {got}")
    k = int(rec_records.shape[1])
    if int(rec_records.shape[0]) != g:
        raise ValueError(f"{what}: counts rows are {g} wide, rec_records holds {int(rec_records.shape[0])} clusters")
    _scan_tensor(what, "rec_records", rec_records, torch.int64, (g, k), dev)
    _scan_tensor(what, "records", records, torch.int64, (n_boot + 1, k), dev)
    lib.call("eeg_dcrnn_boot_records", _p(rec_records), g, k, _p(counts), n_boot, _p(records), _stream(counts))


_define("boot_counts", "(int seed, Tensor(a!) counts) -> ()", _boot_counts_impl, lambda *a: None)
_define("boot_detection", "(Tensor probs, Tensor labels, Tensor? groups, Tensor? losses, Tensor counts, float thresh, int max_cluster, Tensor(a!) ws, "
        "Tensor(b!) records) -> ()", _boot_detection_impl, lambda *a: None)
_define("boot_classification", "(Tensor probs, Tensor labels, Tensor? groups, Tensor counts, int max_cluster, Tensor(a!) ws, Tensor(b!) records) -> ()",
        _boot_classification_impl, lambda *a: None)
_define("boot_records", "(Tensor rec_records, Tensor counts, Tensor(a!) records) -> ()", _boot_records_impl, lambda *a: None)


def boot_counts(num_groups: int, n_boot: int, seed: int, device):
    """The resampling counts of a clustered bootstrap: (n_boot + 1, G) int32 on `device`.  Row 0 is ones (the point estimate); row r >= 1
    is a multinomial draw of G cluster indices with replacement -- draw j is word j % 4 of Philox4x32-10 at the counter (lo(j / 4),
    hi(j / 4), r, 4) under key `seed` and names cluster (word * G) >> 32 (bias at most G / 2^32 per cluster).  A function of (G, n_boot,
    seed) alone: every rank and every run draws the same counts.  One launch, no host synchronisation."""
    g, n = int(num_groups), int(n_boot)
    if not 1 <= g <= BOOT_MAX_GROUPS:
        raise ValueError(f"boot_counts: G={g} clusters outside 1..{BOOT_MAX_GROUPS} (EEG_BOOT_MAX_GROUPS)")
    if not 1 <= n <= BOOT_MAX_REPLICATES:
        raise ValueError(f"boot_counts: n_boot={n} replicates outside 1..{BOOT_MAX_REPLICATES} (EEG_BOOT_MAX_REPLICATES)")
    if not 0 <= int(seed) < 1 << 63:
        raise ValueError(f"boot_counts: seed={seed} outside 0..2^63-1")
    counts = torch.empty((n + 1, g), dtype=torch.int32, device=device)
    torch.ops.eeg_dcrnn.boot_counts(int(seed), counts)
    return counts


def boot_workspace(num_clips: int, device):
    """the scratch of `boot_detection` / `boot_classification` for a pool of `num_clips` clips (eeg_dcrnn_boot_ws_bytes)"""
    if not 1 <= int(num_clips) <= EVAL_MAX_CLIPS:
        raise ValueError(f"boot_workspace: P={num_clips} clips outside 1..{EVAL_MAX_CLIPS} (EEG_EVAL_MAX_CLIPS)")
    return torch.empty((int(_lib.get_lib().query("eeg_dcrnn_boot_ws_bytes", int(num_clips))) + 7) // 8, dtype=torch.int64, device=device)


def boot_check_groups(what, groups, num_clips: int, num_groups: int):
    """Host check of a clustering (one small copy): groups (P,) int32 with 0 <= groups[i] < G.  -> the clips of the largest cluster
    (groups None: every clip its own cluster, 1)."""
    if groups is None:
        if int(num_groups) != int(num_clips):
            raise ValueError(f"{what}: groups is None (every clip its own cluster): counts rows must be P={num_clips} wide, got {num_groups}")
        return 1
    if not torch.is_tensor(groups) or groups.dtype != torch.int32 or tuple(groups.shape) != (int(num_clips),):
        got = f"{groups.dtype} {tuple(groups.shape)}" if torch.is_tensor(groups) else type(groups).__name__
        raise ValueError(f"{what}: groups must be a torch.int32 tensor of shape ({int(num_clips)},), got {got}")
    lo, hi = int(groups.min()), int(groups.max())
    if lo < 0 or hi >= int(num_groups):
        raise ValueError(f"{what}: groups holds cluster ids {lo}..{hi}, outside 0..G-1 = {int(num_groups) - 1}")
    return int(torch.bincount(groups.long(), minlength=1).max())


def boot_detection(probs, labels, groups, counts, thresh: float = 0.5, losses=None, *, ws=None, max_cluster: Optional[int] = None):
    """One int64 record per replicate of a clustered bootstrap of the detection scores: (n_boot + 1, BOOT_DET_WORDS), the words of
    BOOT_RECORD.  probs / labels (P,) float32, groups (P,) int32 cluster ids or None (every clip its own cluster), counts (n_boot + 1,
    G) int32 (`boot_counts`, or explicit), losses (P,) float32 or None.  Clip i weighs counts[r, groups[i]] in replicate r; the words
    are the weighted forms of `eval_metrics`' N, n_pos, n_neg, AUROC numerator and tp / fp / fn / tn at (double)prob > thresh, the bits
    of the float64 average precision and of sum_i w_i * loss_i.  Integer words reproduce bit for bit.  max_cluster: the clips of the
    largest cluster when the caller has validated `groups` already (else checked here on the host: one small copy)."""
    g = int(counts.shape[1]) if torch.is_tensor(counts) and counts.dim() == 2 else 0
    if max_cluster is None:
        max_cluster = boot_check_groups("boot_detection", groups, probs.shape[0] if torch.is_tensor(probs) else 0, g)
    if ws is None and torch.is_tensor(probs) and 1 <= probs.shape[0] <= EVAL_MAX_CLIPS:
        ws = boot_workspace(probs.shape[0], probs.device)
    records = torch.empty((int(counts.shape[0]) if g else 1, BOOT_DET_WORDS), dtype=torch.int64, device=counts.device if g else None)
    torch.ops.eeg_dcrnn.boot_detection(probs, labels, groups, losses, counts, float(thresh), int(max_cluster), ws, records)
    return records


def boot_classification(probs, labels, groups, counts, *, ws=None, max_cluster: Optional[int] = None):
    """The weighted confusion matrix of every replicate: (n_boot + 1, C * C) int64, row = label, column = the first arg-max of the row of
    probs (P, C) float32 (`eval_metrics`' rule; a row it counts as bad is left out).  labels (P,) int64; groups / counts / max_cluster
    as `boot_detection`.  2 <= C <= BOOT_MAX_CLASSES."""
    g = int(counts.shape[1]) if torch.is_tensor(counts) and counts.dim() == 2 else 0
    if max_cluster is None:
        max_cluster = boot_check_groups("boot_classification", groups, probs.shape[0] if torch.is_tensor(probs) else 0, g)
    if ws is None and torch.is_tensor(probs) and 1 <= probs.shape[0] <= EVAL_MAX_CLIPS:
        ws = boot_workspace(probs.shape[0], probs.device)
    c = int(probs.shape[1]) if torch.is_tensor(probs) and probs.dim() == 2 else 1
    records = torch.empty((int(counts.shape[0]) if g else 1, c * c), dtype=torch.int64, device=counts.device if g else None)
    torch.ops.eeg_dcrnn.boot_classification(probs, labels, groups, counts, int(max_cluster), ws, records)
    return records


def boot_records(rec_records, counts):
    """records[r, k] = sum_g counts[r, g] * rec_records[g, k]: the replicates of per-cluster integer records (G, K) int64, e.g.
    `ScanResult.rec_records` with one record per recording.  (n_boot + 1, K) int64, K <= BOOT_MAX_RECORD_WORDS."""
    n = int(counts.shape[0]) if torch.is_tensor(counts) and counts.dim() == 2 else 1
    k = int(rec_records.shape[1]) if torch.is_tensor(rec_records) and rec_records.dim() == 2 else 1
    records = torch.empty((n, k), dtype=torch.int64, device=counts.device if torch.is_tensor(counts) else None)
    torch.ops.eeg_dcrnn.boot_records(rec_records, counts, records)
    return records
