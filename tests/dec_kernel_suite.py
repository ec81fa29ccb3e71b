"""The persistent decoder kernels (csrc/kernels_decoder.h: dec_fwd_persist_kernel<64, M>, dec_bwd_persist_kernel<64, M, DT, CX0>,
instantiated in csrc/dec_inst.cpp / decb_inst.cpp) at every template instance a decoder can reach.  Which instance takes a decoder is
invisible to a parity test -- they compute the same recurrence -- so every case here is ONE DCGRUDecoder forward + backward (operands as
parity_suite.check_decoder_vs_oracle builds them, the oracle's decoder in float64 as the reference) with the event recorder on:
`dec_fwd_persist` and `dec_bwd_persist` must each go out once, as the kernels the case names, and no per-step decoder launch may run,
before outputs, dh0 and every parameter gradient are compared.  The selection rules are restated below from the documented geometry
(DESIGN.md 4.4), not by calling the library; tests/test_dec_kernels.py holds the restatement against the library over the whole grid
and CASES against the enumeration of the restatement: 6 forward and 32 backward instances, one row per backward instance.  Shapes are
the smallest that reach an instance: 2..3 clips of 2..4 steps, except the cases outside the table -- the horizon's edge (64 / 65
steps), WALK_CASES with one clip more than the grid (exactly one workgroup takes a second clip) and DROPOUT_CASES.

`python tests/dec_kernel_suite.py` evaluates the reference in fp32 on the host (the level of a correct fp32 evaluation: it must stay
below a fifth of every tolerance, else the operands are badly scaled); `--device cuda|cpu --out FILE` adds the kernels' errors and
writes the table of profiles/dec_kernel_parity.txt."""
import os
import random
import sys

if __name__ == "__main__":                # (as a script: the paths tests/conftest.py sets up)
    sys.path[1:1] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")]
import numpy as np
import torch

import cases
import parity_suite as ps
import quad_gemm_suite as qg
from oracle import dcrnn_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GRAD_TOL = qg.GRAD_TOL
H, MS = 64, (1, 2, 3, 4, 5, 7)
DEC_GRID = 256                                                        # one workgroup per clip up to one per CU
PER_STEP_ROLES = ("dec_gemm_nn", "dec_seq_", "dec_diffuse_", "dec_gemm_dx")
LAP, RW, DUAL = "laplacian", "random_walk", "dual_random_walk"        # M = k + 1, k + 1, 2k + 1


def hops(filt, order):
    return (2 if filt == DUAL else 1) * order + 1


# ---- kernel symbols as the event recorder spells them ---------------------------------------------------------------------------
def fwd(m):
    return f"dec_fwd_persist_kernel<64, {m}>"


def bwd(m, dt, cx0):
    return f"dec_bwd_persist_kernel<64, {m}, {dt}, {cx0}>"


# ---- the selection rules, restated (nothing here calls the library) ------------------------------------------------
# The kernels' LDS tiles have 20 node rows; a hop polynomial is one zero-padded 32 x 32 matrix at a row stride of 34 floats; a CU has
# 160 KiB of LDS.  Row strides of the plain tiles are padded to 4 mod 64 floats (conflict-free fragment reads).
ROWS, P_FLOATS, LDS_BYTES = 20, 32 * 34, 160 * 1024
MAX_NODES, MAX_LAYERS, MAX_STEPS, MAX_DOUT = 20, 4, 64, 256


def round_up(a, b):
    return (a + b - 1) // b * b


def stride_4_mod_64(k):
    return k + (4 - k % 64) % 64


def quad_chunks(m, dout):
    """16-deep chunks of the layer-0 x-part in its quad pack: the whole chunks of each of the m hop slots, then the leftover 16-byte
    pieces of all slots gathered four to a chunk, padded to a multiple of four chunks (the weight ring)"""
    return round_up(m * (dout // 16) + (m * ((dout // 4) % 4) + 3) // 4, 4)


def fwd_lds_bytes(m, layers, dout):
    """hop polynomials, one state tile [20][M * 64] per layer, the step-input tile [20][M * round_up(Dout, 16), padded] (or the r*h tile
    [20][M * 64] where that is wider), the dropped top state [20][64], the piece-column table (four ints per chunk)"""
    xs = stride_4_mod_64(m * round_up(dout, 16))
    return 4 * ((m - 1) * P_FLOATS + layers * ROWS * m * H + ROWS * max(xs, m * H) + ROWS * 64 + 4 * quad_chunks(m, dout))


def bwd_lds_bytes(m, layers, dout):
    """hop polynomials, the dC tile [20][M * 64] and the [dR|dU] tile [20][M * 128] with their adjoint hop slots, two output-gradient
    tiles [20][round_up(Dout, 16), padded], per layer the recurrent gradient in lane-linear slots (4 waves x 2 x 64 lanes x float4)"""
    fs = stride_4_mod_64(round_up(dout, 16))
    return 4 * ((m - 1) * P_FLOATS + ROWS * (m * H + m * 2 * H) + 2 * ROWS * fs + layers * 4 * 2 * 256)


def dt_of(dout):
    """k-steps per weight group of the backward's projection transpose: 5 where Dout / 4 is a multiple of 5, else 4; 0: neither"""
    q4 = dout // 4
    return 5 if q4 % 5 == 0 else 4 if q4 % 4 == 0 else 0


def cx0_of(dout):
    """column tiles of layer 0's c1 / c2 packs [hidden | input]: 64 + 128 columns up to 128 outputs, else 64 + Dout rounded up to 64"""
    return (H + (128 if dout <= 128 else round_up(dout, 64))) // 16


def is_persistent(t, n, h, dout, m, layers):
    return (h == H and 1 <= n <= MAX_NODES and 1 <= layers <= MAX_LAYERS and 1 <= t <= MAX_STEPS and m in MS
            and 4 <= dout <= MAX_DOUT and dout % 4 == 0 and dt_of(dout) != 0 and not (m == 7 and dout > 128)
            and fwd_lds_bytes(m, layers, dout) <= LDS_BYTES and bwd_lds_bytes(m, layers, dout) <= LDS_BYTES)


def symbols_of(m, dout):
    """the two instances that take a decoder of m hop matrices and dout outputs, where is_persistent holds"""
    return {"dec_fwd_persist": fwd(m), "dec_bwd_persist": bwd(m, dt_of(dout), cx0_of(dout))}


def reachable_instances():
    """every symbol some persistent decoder runs: hop counts x layers x outputs in multiples of 4 -> (forward set, backward set)"""
    f, b = set(), set()
    for m in MS:
        for layers in range(1, MAX_LAYERS + 1):
            for dout in range(4, MAX_DOUT + 1, 4):
                if is_persistent(1, 1, H, dout, m, layers):
                    s = symbols_of(m, dout)
                    f.add(s["dec_fwd_persist"])
                    b.add(s["dec_bwd_persist"])
    return f, b


# (M, Dout, L) at the last byte of an instance's LDS -> the next shapes out, which must be refused
LDS_EDGES = {
    (4, 192, 4): [(4, 208, 4)],
    (5, 144, 3): [(5, 160, 3)],
    (5, 208, 2): [(5, 220, 2), (5, 224, 2)],
    (7, 128, 1): [(7, 140, 1), (7, 80, 2)],
}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _case(filt, order, dout, layers, n, t, b, act, flags, sup, bwd_sym, dropout=0.0):
    """(filt, order) -> M hop matrices; dout outputs; layers; n nodes; t steps of b clips.  flags: None = fully autoregressive, "host" =
    the reference's coin flips at ratio 0.5 from a `random` seed with mixed outcomes, "device" = the int32[T] flag tensor the kernels
    read when they start (pattern of parity_suite.check_decoder_vs_oracle), "third" = device flags on steps 0, 3, 6, ..  sup: "shared" =
    2-D supports (one graph for all clips), "per_clip" = 3-D."""
    m = hops(filt, order)
    return dict(filt=filt, order=order, m=m, dout=dout, layers=layers, n=n, t=t, b=b, act=act, flags=flags, sup=sup, dropout=dropout,
                expect={"dec_fwd_persist": fwd(m), "dec_bwd_persist": bwd_sym})


# One row per backward instance (M, DT, CX0); the six forward instances follow from M.  relu only at small clip counts (its gradient
# jumps where a pre-activation is within rounding of zero: tests/seq_kernel_suite.py), so the rows the WALK_CASES re-run are tanh.
CASES = {
    # ---- up to 128 outputs: CX0 = 12 ----
    "m1_d48_l1": _case(RW, 0, 48, 1, 5, 3, 2, "tanh", None, "shared", bwd(1, 4, 12)),
    "m1_d120_l4": _case(RW, 0, 120, 4, 19, 3, 3, "relu", "device", "per_clip", bwd(1, 5, 12)),
    "m2_d112_l2": _case(LAP, 1, 112, 2, 19, 3, 2, "tanh", "host", "shared", bwd(2, 4, 12)),            # 7 output tiles: wave 3 has no second one
    "m2_d20_l3": _case(RW, 1, 20, 3, 12, 2, 3, "relu", None, "per_clip", bwd(2, 5, 12)),
    "m3_d64_l4": _case(DUAL, 1, 64, 4, 16, 3, 2, "tanh", "device", "per_clip", bwd(3, 4, 12)),
    "m3_d60_l1": _case(LAP, 2, 60, 1, 20, 4, 2, "relu", "host", "shared", bwd(3, 5, 12)),
    "m4_d96_l2": _case(LAP, 3, 96, 2, 17, 2, 2, "tanh", None, "per_clip", bwd(4, 4, 12)),
    "m4_d100_l3": _case(RW, 3, 100, 3, 20, 3, 2, "relu", "device", "shared", bwd(4, 5, 12)),
    "m5_d128_l3": _case(DUAL, 2, 128, 3, 12, 2, 2, "tanh", None, "per_clip", bwd(5, 4, 12)),
    "m5_d80_l3": _case(DUAL, 2, 80, 3, 5, 3, 2, "relu", "host", "shared", bwd(5, 5, 12)),              # 80 / 4 = 20: divisible by 4 and 5 -> DT = 5
    "m7_d128_l1": _case(DUAL, 3, 128, 1, 19, 3, 2, "relu", None, "per_clip", bwd(7, 4, 12)),           # LDS edge: 162 944 B backward
    "m7_d60_l2": _case(DUAL, 3, 60, 2, 16, 3, 2, "tanh", "device", "shared", bwd(7, 5, 12)),
    # ---- 129 .. 192 outputs: CX0 = 16 ----
    "m1_d144_l4": _case(RW, 0, 144, 4, 20, 2, 2, "tanh", None, "per_clip", bwd(1, 4, 16)),
    "m1_d180_l1": _case(LAP, 0, 180, 1, 17, 4, 3, "relu", "device", "shared", bwd(1, 5, 16)),
    "m2_d192_l3": _case(LAP, 1, 192, 3, 5, 3, 2, "tanh", "host", "per_clip", bwd(2, 4, 16)),
    "m2_d140_l2": _case(RW, 1, 140, 2, 19, 2, 3, "relu", None, "shared", bwd(2, 5, 16)),
    "m3_d176_l2": _case(RW, 2, 176, 2, 12, 3, 2, "tanh", "device", "per_clip", bwd(3, 4, 16)),
    "m3_d160_l4": _case(DUAL, 1, 160, 4, 17, 2, 2, "relu", None, "shared", bwd(3, 5, 16)),             # 160 / 4 = 40: the DT tie again
    "m4_d192_l4": _case(RW, 3, 192, 4, 16, 2, 2, "tanh", None, "per_clip", bwd(4, 4, 16)),             # LDS edge: 162 624 B forward
    "m4_d140_l1": _case(LAP, 3, 140, 1, 12, 3, 2, "relu", "host", "shared", bwd(4, 5, 16)),
    "m5_d144_l3": _case(DUAL, 2, 144, 3, 20, 2, 2, "tanh", None, "shared", bwd(5, 4, 16)),             # LDS edge
    "m5_d180_l2": _case(DUAL, 2, 180, 2, 17, 3, 2, "relu", "device", "per_clip", bwd(5, 5, 16)),
    # ---- 193 .. 256 outputs: CX0 = 20 ----
    "m1_d256_l4": _case(LAP, 0, 256, 4, 16, 2, 2, "tanh", None, "per_clip", bwd(1, 4, 20)),
    "m1_d220_l2": _case(RW, 0, 220, 2, 19, 3, 3, "relu", "host", "shared", bwd(1, 5, 20)),
    "m2_d208_l1": _case(RW, 1, 208, 1, 20, 3, 2, "tanh", None, "per_clip", bwd(2, 4, 20)),
    "m2_d240_l3": _case(LAP, 1, 240, 3, 16, 4, 2, "relu", "device", "shared", bwd(2, 5, 20)),
    "m3_d224_l3": _case(LAP, 2, 224, 3, 19, 3, 2, "tanh", "host", "shared", bwd(3, 4, 20)),
    "m3_d200_l3": _case(DUAL, 1, 200, 3, 5, 2, 3, "relu", None, "per_clip", bwd(3, 5, 20)),
    "m4_d256_l3": _case(LAP, 3, 256, 3, 17, 3, 2, "tanh", "device", "per_clip", bwd(4, 4, 20)),
    "m4_d200_l2": _case(RW, 3, 200, 2, 5, 3, 2, "relu", "host", "shared", bwd(4, 5, 20)),
    "m5_d208_l2": _case(DUAL, 2, 208, 2, 12, 2, 2, "tanh", None, "per_clip", bwd(5, 4, 20)),           # LDS edge
    "m5_d240_l1": _case(DUAL, 2, 240, 1, 20, 4, 3, "tanh", "device", "shared", bwd(5, 5, 20)),
}

# the horizon: the kernels keep the flags of a decoder in one 64-bit mask (`1ull << t`); 64 steps is the last persistent horizon
T_CASES = {
    "t64_autoregressive": _case(RW, 0, 16, 1, 3, 64, 2, "tanh", None, "shared", bwd(1, 4, 12)),
    "t64_flags": _case(RW, 0, 16, 1, 3, 64, 2, "tanh", "third", "shared", bwd(1, 4, 12)),              # step 63 is flagged: bit 63 of the mask
}
# 65 steps: not persistent -- the per-step launches run (flags as a host tuple: device flags need the persistent kernels)
T65_CASES = {name.replace("t64", "t65"): dict(c, t=65, expect=None) for name, c in T_CASES.items()}
# one clip more than the grid: exactly one workgroup walks on to a second clip.  Also run with the cotangent on three clips only.
WALK_CASES = {name + "_walk": dict(CASES[name], b=DEC_GRID + 1, t=2) for name in ("m4_d96_l2", "m5_d208_l2", "m1_d256_l4")}
# nn.Dropout(0.5) in front of the projection: masks drawn inside the kernels, recomputed in the backward
DROPOUT_CASES = {name + "_dropout": dict(CASES[name], dropout=0.5) for name in ("m4_d100_l3", "m3_d224_l3")}
DROPOUT_SEED, DROPOUT_OFFSET = 20240917, 3
ALL_CASES = {**CASES, **T_CASES, **T65_CASES, **WALK_CASES, **DROPOUT_CASES}

# the emulator's share: every M, both DT, all three CX0, L = 1 and L = 4, every M = 4 row; and the 64-step case with flags
EMU_CASES = ("m1_d48_l1", "m2_d20_l3", "m3_d64_l4", "m4_d96_l2", "m4_d100_l3", "m5_d80_l3", "m7_d60_l2", "m1_d180_l1", "m4_d192_l4", "m4_d140_l1",
             "m2_d208_l1", "m4_d256_l3", "m4_d200_l2", "t64_flags")


def sparse_clips(b):
    """first clip, the last clip of the grid's first round, the one clip of its second round (= the last clip: b = grid + 1)"""
    return sorted({0, DEC_GRID - 1, DEC_GRID, b - 1})


def _mixed(mask):
    return any(mask[:-1]) and not all(mask[:-1])


def flag_mask(case):
    """-> (per-step teacher-forcing flags or None, the `random` seed that replays them on the host or None)"""
    t = case["t"]
    if case["flags"] is None:
        return None, None
    if case["flags"] == "third":
        return [i % 3 == 0 for i in range(t)], None
    if case["flags"] == "device":
        for phase in range(5):
            mask = [(3 * i + phase) % 5 in (0, 3) for i in range(t)]
            if _mixed(mask):
                return mask, None
    for seed in range(64):                       # "host": the coin flips of model.py:194-200 at ratio 0.5
        random.seed(seed)
        mask = [random.random() < 0.5 for _ in range(t)]
        if _mixed(mask):
            return mask, seed
    raise AssertionError(f"no mixed flags at T = {t}")


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------
_ADJ = []


def _adj3d():
    if not _ADJ:
        _ADJ.append(np.load(os.path.join(HERE, "golden", "adj_mx_3d.npy")))
    return _ADJ[0]


def make_supports(case, g):
    filt, n, b = case["filt"], case["n"], case["b"]
    count = b if case["sup"] == "per_clip" else 1
    sup = cases.supports_for(filt, _adj3d(), count) if n == 19 else ps.random_supports(n, count, filt, g)
    return sup if case["sup"] == "per_clip" else [s[0] for s in sup]


def make_operands(case, seed=0):
    """as parity_suite.check_decoder_vs_oracle: the reference's initialisation with random biases, targets, initial states, a
    cotangent; supports of the montage's distance / correlation graphs at 19 nodes and random directed graphs elsewhere"""
    g = torch.Generator().manual_seed(seed)
    cfg = orc.DCRNNConfig(filter_type=case["filt"], input_dim=case["dout"], output_dim=case["dout"], rnn_units=H, num_rnn_layers=case["layers"],
                          dcgru_activation=case["act"], num_nodes=case["n"], max_diffusion_step=case["order"])
    params = {k: v for k, v in orc.init_params(cfg, "ssl", seed=seed).items() if k.startswith("decoder.")}
    for k in params:
        if k.endswith("biases") and not any(params[k] is params[q] for q in params if q < k):
            params[k].copy_(0.1 * torch.randn(params[k].shape, generator=g))
    t, b, n, dout = case["t"], case["b"], case["n"], case["dout"]
    sup = make_supports(case, g)
    mask, flag_seed = flag_mask(case)
    return dict(cfg=cfg, params=params, sup=sup, targets=torch.randn(t, b, n, dout, generator=g), h0=0.5 * torch.randn(case["layers"], b, n * H, generator=g),
                wout=torch.randn(t, b, n * dout, generator=g), mask=mask, flag_seed=flag_seed)


def dropout_masks(case, dtype=torch.float64):
    """the keep-mask x 1 / (1 - p) factors (T, B, N, H) of a decoder seeded (DROPOUT_SEED, DROPOUT_OFFSET), from the documented function
    of the generator pair (parity_suite.expected_mask: Philox4x32-10 on the host)"""
    if not case["dropout"]:
        return None
    t, b, n = case["t"], case["b"], case["n"]
    return torch.from_numpy(ps.expected_mask(DROPOUT_SEED, DROPOUT_OFFSET, t * b * n * H, case["dropout"])).view(t, b, n, H).to(dtype)


def reference(case, op, cots, dtype=torch.float64):
    """orc.decoder_forward on operands of `dtype` -> (outputs, [{name: gradient} per cotangent]); shared tensors stay shared"""
    uniq, po = {}, {}
    for k, v in op["params"].items():
        if v.data_ptr() not in uniq:
            uniq[v.data_ptr()] = v.detach().to(dtype).requires_grad_(True)
        po[k] = uniq[v.data_ptr()]
    h0 = op["h0"].detach().to(dtype).requires_grad_(True)
    out = orc.decoder_forward(po, op["cfg"], op["targets"].to(dtype), h0, [s.to(dtype) for s in op["sup"]], op["mask"], dropout_masks=dropout_masks(case, dtype))
    leaves = [h0] + list(uniq.values())
    names = ["dh0"] + [next(k for k in po if po[k] is v)[len("decoder."):] for v in uniq.values()]
    grads = []
    for i, w in enumerate(cots):
        gs = torch.autograd.grad((out * w.to(dtype)).sum(), leaves, retain_graph=i + 1 < len(cots))
        grads.append(dict(zip(names, gs)))
    return out.detach(), grads


_REF_CACHE = {}


def cached_reference(name, seed=0):
    """(operands, cotangents, reference outputs, reference gradients per cotangent) of a case, computed once per process: the dense
    cotangent and -- WALK_CASES -- the one that lives on sparse_clips only"""
    key = (name, seed)
    if key not in _REF_CACHE:
        case = ALL_CASES[name]
        op = make_operands(case, seed)
        cots = [op["wout"]]
        if name in WALK_CASES:
            keep = torch.zeros(case["b"], dtype=torch.bool)
            keep[sparse_clips(case["b"])] = True
            cots.append(op["wout"] * keep.view(1, -1, 1))
        out, grads = reference(case, op, cots)
        _REF_CACHE[key] = (op, cots, out, grads)
    return _REF_CACHE[key]


def errors(out, grads, ref_out, ref_grads):
    errs = {"out": ps.rel_err(out.detach().cpu().numpy(), ref_out.numpy())}
    for k, g in grads.items():
        ref = ref_grads[k].numpy()
        errs[k] = float(abs(g.detach().cpu().double().numpy() - ref).max() / max(abs(ref).max(), 1e-6))
    return errs


def yardstick(name, seed=0):
    """the reference's own arithmetic in fp32 on the host against the float64 reference: {tensor: error} for the dense cotangent"""
    op, cots, ref_out, ref_grads = cached_reference(name, seed)
    out, grads = reference(ALL_CASES[name], op, cots[:1], dtype=torch.float32)
    return errors(out, grads[0], ref_out, ref_grads[0])


# ---- the decoder under test -----------------------------------------------------------------------------------------------------
def run_decoder(case, op, wout, device):
    """-> run(): one forward + backward of DCGRUDecoder on `device` -> (outputs, {name: gradient}); run.forward_only(): the forward under
    torch.no_grad().  Every call replays the same flags (host: the same `random` seed) and, under dropout, the same generator pair."""
    from eeg_gnn_ssl_amd import DCGRUDecoder
    dec = DCGRUDecoder(input_dim=case["dout"], max_diffusion_step=case["order"], num_nodes=case["n"], hid_dim=H, output_dim=case["dout"],
                       num_rnn_layers=case["layers"], dcgru_activation=case["act"], filter_type=case["filt"], dropout=case["dropout"])
    ps.load(dec, {k[len("decoder."):]: v for k, v in op["params"].items()}, device)
    dec.train()
    targets, h0, woutd, sup = op["targets"].to(device), op["h0"].to(device), wout.to(device), [s.to(device) for s in op["sup"]]
    mask, persistent = op["mask"], case["expect"] is not None
    kw = {}
    if mask is not None and op["flag_seed"] is not None:
        kw = dict(teacher_forcing_ratio=0.5)                                               # the module draws the flags itself
    elif mask is not None and persistent:
        kw = dict(teacher_flags=torch.tensor([1 if v else 0 for v in mask], dtype=torch.int32, device=device))
    elif mask is not None:
        kw = dict(teacher_flags=tuple(mask))                                               # (per-step path: flags on the host)

    def forward(h0d):
        if case["dropout"]:
            dec.set_dropout_seed(DROPOUT_SEED, DROPOUT_OFFSET)
        if op["flag_seed"] is not None:
            random.seed(op["flag_seed"])
        return dec(targets, h0d, sup, **kw)

    def run():
        dec.zero_grad()
        h0d = h0.clone().requires_grad_(True)
        out = forward(h0d)
        (out * woutd).sum().backward()
        grads = {"dh0": h0d.grad.clone()}
        grads.update({k: p.grad.clone() for k, p in dec.named_parameters()})
        return out.detach().clone(), grads

    def forward_only():
        with torch.no_grad():
            return forward(h0)
    run.forward_only = forward_only
    run.decoder = dec
    return run


def assert_ran(ran, case, what):
    """the recorder's {role: {symbol: launches}} of ONE forward + backward: the two persistent roles went out once each, as the expected
    kernels, and no per-step decoder launch ran; a case without `expect` (65 steps): the other way round"""
    per_step = {r: sum(s.values()) for r, s in ran.items() if r.startswith(PER_STEP_ROLES)}
    got = {role: ran.get(role, {}) for role in ("dec_fwd_persist", "dec_bwd_persist")}
    if case["expect"] is None:
        assert got == {"dec_fwd_persist": {}, "dec_bwd_persist": {}}, f"{what}: a persistent kernel ran beyond its horizon: {got}"
        steps = case["t"] * case["layers"]
        assert per_step.get("dec_seq_fwd") == steps and per_step.get("dec_seq_bwd") == steps, f"{what}: per-step launches {per_step}"
        return
    want = {role: {sym: 1} for role, sym in case["expect"].items()}
    assert got == want, f"{what}: persistent decoder kernels that ran {got}, expected {want}"
    assert not per_step, f"{what}: per-step decoder launches beside the persistent kernels: {per_step}"


def check_case(name, device, sparse=False, seed=0, report=None):
    """One case: the decoder on `device` against the float64 reference (outputs under assert_close, dh0 and every parameter gradient
    under assert_close_scaled(tol=5e-5)), after the proof that the expected kernels ran; then -- on the MI355X -- the forward once more
    under torch.no_grad(), bit for bit the same outputs.  sparse (WALK_CASES): the cotangent lives on sparse_clips only, so that a clip
    dropped, doubled or misplaced in the walk is measured against three clips' worth of gradient, and no other clip's initial state
    may receive one bit of it.  Dropout: the masks of the generator pair go to the reference, ops.dropout_mask must return the same
    ones, and the generator must have advanced by one counter per four elements of the T top states."""
    from eeg_gnn_ssl_amd import ops
    case = ALL_CASES[name]
    assert not sparse or name in WALK_CASES
    dims = (case["t"], case["b"], case["n"], H, case["dout"], case["m"], case["layers"])
    assert ops.decoder_is_persistent(*dims) is (case["expect"] is not None), (name, dims)
    op, cots, ref_out, ref_grads = cached_reference(name, seed)
    which = 1 if sparse else 0
    run = run_decoder(case, op, cots[which], device)
    if device != "cpu":
        run()                                                                             # (first call: allocations)
    res = {}
    ran = ps.kernels_run(lambda: res.update(res=run()))
    out, grads = res["res"]
    what = f"{name}{' (sparse)' if sparse else ''} T={case['t']} B={case['b']} N={case['n']}"
    assert_ran(ran, case, what)
    if case["dropout"]:
        groups = case["t"] * case["b"] * case["n"] * H // 4
        assert run.decoder.dropout_rng_state() == (DROPOUT_SEED, DROPOUT_OFFSET + groups), f"{what}: generator state {run.decoder.dropout_rng_state()}"
        used = torch.tensor([DROPOUT_SEED, DROPOUT_OFFSET], dtype=torch.int64, device=device)
        drawn = ops.dropout_mask(used, 4 * groups, case["dropout"]).view(case["t"], case["b"], case["n"], H).cpu()
        assert torch.equal(drawn, dropout_masks(case, torch.float32)), f"{what}: ops.dropout_mask differs from the documented masks"
        assert all(not torch.equal(drawn[t], drawn[0]) for t in range(1, case["t"])), f"{what}: the same mask at two steps"
    errs = errors(out, grads, ref_out, ref_grads[which])
    print(f"dec-kernel {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"dec-kernel {what} ran: " + "; ".join(f"{role} = {sym}" for role in ("dec_fwd_persist", "dec_bwd_persist") for sym in ran.get(role, {})))
    if report is not None:
        report[what] = errs
    assert set(grads) == set(ref_grads[which]), (sorted(grads), sorted(ref_grads[which]))
    ps.assert_close(out.cpu().numpy(), ref_out.numpy(), f"{what}: outputs")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[which][k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
    if sparse:                                    # clips without a cotangent: not one bit of gradient reaches their initial states
        keep = sparse_clips(case["b"])
        rest = [i for i in range(case["b"]) if i not in keep]
        assert not grads["dh0"][:, rest].any(), f"{what}: dh0 of a clip without a cotangent is not zero"
        assert grads["dh0"][:, keep].abs().amax(dim=(0, 2)).min() > 0, f"{what}: a clip with a cotangent has no gradient"
    elif device != "cpu":                         # (the emulator's share stays at a few seconds a case: one forward + backward)
        again = run.forward_only()
        assert torch.equal(again, out), f"{what}: the forward under no_grad differs from the training forward"
    return errs, ran


# ---- yardstick and parity table -------------------------------------------------------------------------------------------------
def worst_fractions(errs):
    """(outputs, gradients) as fractions of their tolerances"""
    return errs["out"] / ps.TOL, max(v for k, v in errs.items() if k != "out") / GRAD_TOL


def _row(label, errs, ran=None):
    o, g = worst_fractions(errs)
    worst = max((k for k in errs if k != "out"), key=lambda k: errs[k])
    syms = "" if not ran else "  " + " + ".join(sym for role in ("dec_fwd_persist", "dec_bwd_persist") for sym in ran.get(role, {"(per step)": 1}))
    return f"{label:<42}{o:>9.3f}{g:>9.3f}  {worst:<46}{syms}"


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[-1])
    ap.add_argument("--device", choices=("cuda", "cpu"))
    ap.add_argument("--out")
    ap.add_argument("--cases", nargs="*")
    a = ap.parse_args(argv)
    torch.set_num_threads(16)
    names = a.cases or ([n for n in ALL_CASES if n in EMU_CASES] if a.device == "cpu" else list(ALL_CASES))
    if a.device == "cpu":
        import emu_support
        emu_support.install_emulator()
    lines = [f"{'case (errors as fractions of tolerance)':<42}{'outputs':>9}{'grads':>9}  {'worst gradient':<46}  kernels"]
    worst = 0.0
    for name in names:
        yard = yardstick(name)
        worst = max(worst, *worst_fractions(yard))
        lines.append(_row(f"{name}  fp32 host", yard))
        shown = 1
        if a.device:
            for sparse in (False, True) if name in WALK_CASES else (False,):
                rep = {}
                _, ran = check_case(name, a.device, sparse=sparse, report=rep)
                where = ("MI355X" if a.device == "cuda" else "emulator") + (" sparse" if sparse else "")
                lines.append(_row(f"{'':<{len(name)}}  {where}", next(iter(rep.values())), ran))
                shown += 1
        print("\n".join(lines[-shown:]), flush=True)
    lines.append(f"worst fp32 yardstick / tolerance: {worst:.3f} (must stay below 0.2)")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if worst < 0.2 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
