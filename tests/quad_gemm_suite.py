"""The persistent whole-block GEMMs of csrc/kernels_gemm_q.h (gemm_nnr_kernel, gemm_tnq_kernel, gemm_tnq_pair_kernel) at every template
instance a product build can reach.  They take the hoisted GEMMs of a layer on the general path from 256 rows per CU on
(gemm_launch.h quad_min_rows), so every case here is ONE DCGRU layer with just enough rows for the device it runs on, against a
float64 evaluation of the same layer (the oracle's dtype-generic cell on .double() operands): hidden sequence, input gradient, dh0 and
the four parameter gradients.  The event recorder proves which kernel took each GEMM (`parity_suite.kernels_run`); the plan driver of
tests/emu says, without a GPU, which instances are reachable at all, and CASES must cover exactly that set.  Run by
tests/test_quad_gemm.py on the MI355X library, and at small row counts (dev knob 2) by tests/test_emu_parity.py on the emulator."""
import math
import os
import subprocess

import torch

import parity_suite as ps
from oracle import dcrnn_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "eeg_gnn_ssl_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NO_KNOBS = "0 0 0 0 0 0 0 0"
GRAD_TOL = 5e-5                       # every gradient, relative to the tensor's maximum (as parity_suite.check_vs_oracle_random)

# ---- kernel symbols as the event recorder spells them ---------------------------------------------------------------------------
NNR = "gemm_nnr_kernel<4, 2>"


def _b(v):
    return "true" if v else "false"


def tnq(kt, ot, bt=False, planar=False):
    return f"gemm_tnq_kernel<{kt}, {ot}, 16, {_b(bt)}, {_b(planar)}, false>"


def pair(kt, planar):
    return f"gemm_tnq_pair_kernel<{kt}, 16, {_b(planar)}>"


def nn_dma(nctw, kc):
    return f"gemm_nn_dma_kernel<{nctw}, {kc}, 2>"


def nn_staged(nctw, kc):
    return f"gemm_nn_kernel<{nctw}, {kc}>"


def tn_dma(nctw, rc, wk=2):
    return f"gemm_tn_dma_kernel<2, {nctw}, {rc}, {wk}>"


def tn_staged(nctw):
    return f"gemm_tn_kernel<{nctw}>"


def is_quad(symbol):
    return symbol.startswith(("gemm_nnr_kernel", "gemm_tnq_kernel", "gemm_tnq_pair_kernel"))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# h, (filter, k) -> M hop matrices, fin, bm (the layer is handed the transposed view of a batch-major tensor), n nodes, rows = (mod, res):
# R = T*B*n is the smallest value >= 256 rows per CU with R % mod == res.  expect: role -> symbol of the kernel that takes that GEMM
# (the h-part roles are gemm_tn_h when the pair kernel runs, gemm_tn_hg / gemm_tn_hc when not).  h0: a non-zero initial state;
# lengths: ragged clip lengths (cotangent past a clip's length is zero, and the state at its last step gets one of its own).
CASES = {
    # M = 1: no hop planes, one 64-wide plane per TN k-block (planar KT = 2 at all three widths); nnr with one segment
    "m1_planar": dict(h=64, filt="laplacian", k=0, fin=64, bm=False, n=19, rows=(128, 0), act="tanh", h0=False, lengths=False,
                      expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(2, 16), "gemm_tn_x": tnq(2, 6, planar=True),
                              "gemm_tn_hg": tnq(2, 4, planar=True), "gemm_tn_hc": tnq(2, 2, planar=True)}),
    # M = 2: two planes per k-block (planar KT = 4); the pair kernel has no such instance: three separate launches
    "m2_planar": dict(h=64, filt="laplacian", k=1, fin=64, bm=False, n=19, rows=(128, 0), act="relu", h0=True, lengths=False,
                      expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(4, 16), "gemm_tn_x": tnq(4, 6, planar=True),
                              "gemm_tn_hg": tnq(4, 4, planar=True), "gemm_tn_hc": tnq(4, 2, planar=True)}),
    # M = 4: the h-parts are planar KT = 4 with two k-blocks; the 48-wide x-part (K = 192) goes through per-lane pointers in 4-tile
    # k-blocks; M * Fin = 192 = one whole column block: dX through nnr
    "m4_mixed": dict(h=64, filt="laplacian", k=3, fin=48, bm=False, n=19, rows=(128, 0), act="tanh", h0=False, lengths=True,
                     expect={"gemm_nn_xw": NNR, "gemm_nn_dx": NNR, "gemm_tn_x": tnq(4, 6),
                             "gemm_tn_hg": tnq(4, 4, planar=True), "gemm_tn_hc": tnq(4, 2, planar=True)}),
    # M = 7, Fin = 20: one whole chunk per plane + seven leftover pieces = two tail chunks of nnr; K = 448 of the h-parts in three
    # 160-wide k-blocks, the last one padded
    "m7_tails": dict(h=64, filt="dual_random_walk", k=3, fin=20, bm=True, n=19, rows=(128, 0), act="tanh", h0=True, lengths=False,
                     expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(5, 16), "gemm_tn_x": tnq(5, 6, bt=True), "gemm_tn_h": pair(5, False)}),
    # the smallest K of the batch-major x-part: 60 columns in one 4-tile k-block
    "bt_k4": dict(h=64, filt="laplacian", k=2, fin=20, bm=True, n=19, rows=(128, 0), act="relu", h0=False, lengths=True,
                  expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(2, 16), "gemm_tn_x": tnq(4, 6, bt=True), "gemm_tn_h": pair(6, True)}),
    # a second layer at M = 5 (Fin = H = 64, time-major): five planes are not planar, K = 320 is two exact 160-wide k-blocks of the
    # per-lane-pointer kernel, x-part and paired h-parts alike
    "m5_layer1": dict(h=64, filt="dual_random_walk", k=2, fin=64, bm=False, n=19, rows=(128, 0), act="tanh", h0=False, lengths=False,
                      expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(5, 16), "gemm_tn_x": tnq(5, 6), "gemm_tn_h": pair(5, False)}),
    # M * Fin = 384: dX through nnr with two 192-column blocks (gridDim.y = 2); the x-part TN has K = 384
    "dx_wide": dict(h=64, filt="laplacian", k=1, fin=192, bm=False, n=19, rows=(128, 0), act="tanh", h0=False, lengths=False,
                    expect={"gemm_nn_xw": NNR, "gemm_nn_dx": NNR, "gemm_tn_x": tnq(4, 6),
                            "gemm_tn_hg": tnq(4, 4, planar=True), "gemm_tn_hc": tnq(4, 2, planar=True)}),
    # 32 units: only the gate problem of the h-part (64 columns of 32-wide planes) is covered by the quad kernel; the candidate, the
    # x-part and both NN GEMMs stay on the split kernels -- a mixed cell
    "h32_m3": dict(h=32, filt="laplacian", k=2, fin=36, bm=False, n=19, rows=(128, 0), act="tanh", h0=True, lengths=False,
                   expect={"gemm_nn_xw": nn_staged(6, 4), "gemm_nn_dx": nn_dma(4, 16), "gemm_tn_x": tn_dma(4, 32),
                           "gemm_tn_hg": tnq(4, 2), "gemm_tn_hc": tn_staged(1)}),
    "h32_m5": dict(h=32, filt="dual_random_walk", k=2, fin=36, bm=False, n=19, rows=(128, 0), act="relu", h0=False, lengths=True,
                   expect={"gemm_nn_xw": nn_staged(6, 4), "gemm_nn_dx": nn_dma(6, 16), "gemm_tn_x": tn_dma(4, 32),
                           "gemm_tn_hg": tnq(5, 2), "gemm_tn_hc": tn_staged(1)}),
    # R = 256 rows per CU exactly (32 nodes): the first row count the quad kernels take; every nnr workgroup owns one 128-row tile
    "at_threshold": dict(h=64, filt="laplacian", k=2, fin=64, bm=False, n=32, rows=(128, 0), act="tanh", h0=False, lengths=False,
                         expect={"gemm_nn_xw": NNR, "gemm_nn_dx": NNR, "gemm_tn_x": tnq(6, 6, planar=True), "gemm_tn_h": pair(6, True)}),
    # R % 128 = 48: a partial last 128-row tile of nnr, a short last row split of the TN kernels
    "ragged_128": dict(h=64, filt="dual_random_walk", k=2, fin=100, bm=True, n=19, rows=(128, 48), act="tanh", h0=False, lengths=False,
                       expect={"gemm_nn_xw": NNR, "gemm_nn_dx": nn_dma(4, 16), "gemm_tn_x": tnq(4, 6, bt=True), "gemm_tn_h": pair(5, False)}),
    # R % 16 = 6: nnr with a ragged last 16-row tile on both NN GEMMs; the quad TN kernel needs whole 16-row chunks: all three TNs on
    # the split kernels
    "ragged_16": dict(h=64, filt="laplacian", k=2, fin=64, bm=False, n=19, rows=(16, 6), act="tanh", h0=False, lengths=False,
                      expect={"gemm_nn_xw": NNR, "gemm_nn_dx": NNR, "gemm_tn_x": tn_dma(6, 16),
                              "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
}
SPARSE_CASES = ("m2_planar", "h32_m5", "ragged_128")      # also run with a cotangent on three clips only (check_case(sparse=True))
ROLES = ("gemm_nn_xw", "gemm_nn_dx", "gemm_tn_x", "gemm_tn_h", "gemm_tn_hg", "gemm_tn_hc")


def hops(case):
    return (2 if case["filt"] == "dual_random_walk" else 1) * case["k"] + 1      # (laplacian, random_walk: one support)


# ---- what a layer plans: the calls of csrc/api.cpp restated, answered by the plan driver ------------------------------------------
def build_plan_driver(out_dir, dev=True):
    """tests/emu/gemm_plan_driver.cpp compiled as tests/test_gemm_plans.py does (host code only) -> path of the executable.  dev=False:
    without -DEEG_DEV, as the product library sees the headers (no probe instantiations)"""
    exe = os.path.join(str(out_dir), "gemm_plan_driver")
    subprocess.check_call([CLANG if os.path.exists(CLANG) else "clang++", "-x", "c++", "-std=c++17", "-O1", "-g", "-DEEG_PLATFORM_HEADER=\"platform_emu.h\""] +
                          (["-DEEG_DEV"] if dev else []) + ["-I", os.path.join(HERE, "emu"), "-I", CSRC, "-Wno-unused-function", "-Wno-unknown-attributes",
                           os.path.join(HERE, "emu", "gemm_plan_driver.cpp"), "-o", exe])
    return exe


def layer_calls(h, m, fin, r, bm, cus, knobs=NO_KNOBS):
    """the six driver lines of one layer's hoisted GEMMs, as layer_fwd / layer_bwd / bwd_ws of api.cpp build their calls: the x-part
    NN, the dX NN, the three weight-gradient TNs (offered to the quad kernel) and the pair question.  bm: the input is batch-major AND
    read through the row map (eeg_dcrnn_batch_major_ok == 2: the LDS-DMA kernels apply to Fin; else Python hands in a time-major copy)"""
    row_map = int(bool(bm) and (fin % 16 == 0 or fin % 20 == 0))
    has_bxq = int((3 * h) % 192 == 0)                   # pack_cell.h: the quad-ordered packs exist for whole 192-column blocks
    has_bxtq = int((m * fin) % 192 == 0)
    return [f"nn {m} {fin} {r} {3 * h // 16} {3 * h} {3 * h} {row_map} {has_bxq} 0 {cus} {knobs}",
            f"nn 1 {3 * h} {r} {(m * fin + 15) // 16} {m * fin} {m * fin} 0 {has_bxtq} 0 {cus} {knobs}",
            f"tn {m} {fin} {r} {3 * h} {row_map} 1 {cus} {knobs}",
            f"tn {m} {h} {r} {2 * h} 0 1 {cus} {knobs}",
            f"tn {m} {h} {r} {h} 0 1 {cus} {knobs}",
            f"pair {m} {h} {r} {cus} {knobs}"]


def _nn_symbol(line):
    kind, t1, t2, t3 = (int(v) for v in line.split()[:4])
    assert line.split()[-1] == "0", line
    return [NNR, nn_dma(t1, t2), nn_staged(t1, t2)][kind]


def _tn_symbol(line, row_map):
    f = [int(v) for v in line.split()]
    kind, t1, t2, t3 = f[:4]
    assert f[-1] == 0, line
    if kind == 0:
        return tnq(t1, t2, bt=bool(row_map) and not t3, planar=bool(t3))
    return tn_dma(t1, t2) if kind == 1 else tn_dma(t1, t2, 4) if kind == 2 else tn_staged(t1)


def planned(exe, layers):
    """layers: list of (h, m, fin, r, bm, cus[, knobs]) -> per layer ({role: symbol}, rows per split of the x-part and gate TNs)"""
    lines = [ln for lay in layers for ln in layer_calls(*lay)]
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    res = []
    for i, lay in enumerate(layers):
        o, row_map = out[6 * i:6 * i + 6], layer_calls(*lay)[0].split()[7] == "1"
        roles = {"gemm_nn_xw": _nn_symbol(o[0]), "gemm_nn_dx": _nn_symbol(o[1]), "gemm_tn_x": _tn_symbol(o[2], row_map)}
        if o[5] == "1":
            f = [int(v) for v in o[3].split()]
            roles["gemm_tn_h"] = pair(f[1], bool(f[3]))
        else:
            roles["gemm_tn_hg"], roles["gemm_tn_hc"] = _tn_symbol(o[3], False), _tn_symbol(o[4], False)
        res.append((roles, {"gemm_tn_x": int(o[2].split()[5]), "gemm_tn_hg": int(o[3].split()[5])}))
    return res


def reachable_instances(exe, cus=256):
    """every quad instance some supported layer reaches at the threshold row count: 16 / 32 / 64 units, every supported hop count, every
    input width up to 516, both layouts, no dev knobs"""
    r = 256 * cus
    layers = [(h, m, fin, r, bm, cus) for h in (16, 32, 64) for m in (1, 2, 3, 4, 5, 7) for fin in range(4, 520, 4) for bm in (False, True)]
    return {s for roles, _ in planned(exe, layers) for s in roles.values() if is_quad(s)}


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
def pick_rows(rows_min, n, mod, res, t_min=1):
    """(T, B) with the smallest R = T*B*n >= rows_min that has R % mod == res, B < 384 (below the streamed BPTT kernel's batch)"""
    s = -(-rows_min // n)
    while True:
        if (s * n) % mod == res:
            for t in (12, 8, 16, 13, 14, 10, 9, 11, 15, 6, 4, 5, 7, 3, 2, 1, 17, 18, 19, 20, 24, 32):
                if t >= t_min and s % t == 0 and s // t < 384:
                    return t, s // t
        s += 1


def case_dims(case, rows_min):
    t, b = pick_rows(rows_min, case["n"], *case["rows"], t_min=4 if case["bm"] else 1)    # (the batch-major row map needs T >= 4)
    return t, b, t * b * case["n"]


EMU_KNOB_QUAD = 4                     # dev knob 2 (EEG_TUNE_QUAD) = 4: the quad kernels from one row per CU on
EMU_CUS = 4                           # tests/emu/platform_emu.h platform_num_cus()


def emu_dims(case):
    """(T, B, R) of a case on the emulator: the smallest R above 64 rows (the TN kernels' smallest row split: at least two splits) with
    the case's R % 16, and its R % 128 where that residue is what the case is about (ragged_128; at_threshold's whole tiles).  The other
    cases would need 2432 rows to have 19 nodes AND whole 128-row tiles -- 18 s each on an emulator that runs one lane at a time --
    and run at 304 rows instead: two whole tiles and a partial one."""
    mod, res = case["rows"]
    if mod == 128 and res == 0 and case["n"] % 2 == 1:
        mod = 16
    t, b = pick_rows(65, case["n"], mod, res, t_min=4 if case["bm"] else 1)
    return t, b, t * b * case["n"]


# ---- operands, the float64 reference --------------------------------------------------------------------------------------------
def make_supports(case, b, g):
    """per-clip random directed graphs (the quad table, and every case that does not say otherwise); case["sup"] = "shared": ONE such
    graph in its 2-D form (p_batched = 0 on the general path), "symmetric": the scaled Laplacian of one random undirected graph in its
    2-D form, which the spectral form accepts (tests/seq_kernel_suite.py)"""
    kind = case.get("sup", "per_clip")
    if kind == "per_clip":
        return ps.random_supports(case["n"], b, case["filt"], g)
    if kind == "shared":
        return [s[0].clone() for s in ps.random_supports(case["n"], 1, case["filt"], g)]
    assert kind == "symmetric" and case["filt"] == "laplacian", case
    a = torch.rand(case["n"], case["n"], generator=g)
    a = (0.5 * (a + a.t())).numpy()
    a[range(case["n"]), range(case["n"])] = 1.0
    return orc.compute_supports(a, "laplacian")


def make_operands(case, t, b, seed):
    g = torch.Generator().manual_seed(seed)
    n, h, fin, m = case["n"], case["h"], case["fin"], hops(case)
    kdim = (fin + h) * m
    op = dict(sup=make_supports(case, b, g),
              xb=torch.randn(b, t, n, fin, generator=g),                                   # batch-major storage; the layer sees (T,B,N,Fin)
              h0=0.5 * torch.randn(b, n * h, generator=g) if case["h0"] else None,
              wg=torch.randn(kdim, 2 * h, generator=g) / math.sqrt(kdim), bg=0.1 * torch.randn(2 * h, generator=g),
              wc=torch.randn(kdim, h, generator=g) / math.sqrt(kdim), bc=0.1 * torch.randn(h, generator=g),
              w=torch.randn(t, b, n * h, generator=g), wsel=torch.randn(b, n * h, generator=g),
              lengths=torch.randint(1, t + 1, (b,), generator=g) if case["lengths"] else None)
    if op["lengths"] is not None:
        op["lengths"][0] = t                                                              # (one clip of full length)
        if case.get("len1"):
            op["lengths"][b - 1] = 1                                                      # (and one that ends after its first step)
        op["w"] = op["w"] * (torch.arange(t).view(t, 1, 1) < op["lengths"].view(1, b, 1))
    return op


def sparse_clips(b, n, rps):
    """clip 0, the last clip, and the clip that holds the first row of the second row split (time-major rows (t*B + b)*n + node)"""
    return sorted({0, b - 1, (rps // n) % b})


def _loss(hseq, hsel, w, wsel):
    return (hseq * w).sum() + ((hsel * wsel).sum() if hsel is not None else 0.0)


def reference(case, op, cotangents, dtype=torch.float64):
    """one DCGRU layer in float64 (the oracle's cell over T steps) -> hseq and, per cotangent (w, wsel), the gradients.  (dtype: the
    same evaluation in fp32 is the yardstick of profiles/quad_gemm_parity.txt, not a reference)"""
    n, h, k = case["n"], case["h"], case["k"]
    t, b = op["w"].shape[:2]
    d = {q: op[q].to(dtype).requires_grad_(True) for q in ("xb", "wg", "bg", "wc", "bc")}
    h0 = (op["h0"].to(dtype) if op["h0"] is not None else torch.zeros(b, n * h, dtype=dtype)).requires_grad_(True)
    sup = [s.to(dtype) for s in op["sup"]]
    state, outs = h0, []
    for step in range(t):
        state = orc.dcgru_cell(sup, d["xb"][:, step].reshape(b, -1), state, d["wg"], d["bg"], d["wc"], d["bc"], n, h, k, case["act"])
        outs.append(state)
    hseq = torch.stack(outs)
    hsel = hseq[op["lengths"] - 1, torch.arange(b)] if op["lengths"] is not None else None
    grads = []
    leaves = [d["xb"], h0, d["wg"], d["bg"], d["wc"], d["bc"]]
    for i, (w, wsel) in enumerate(cotangents):
        gs = torch.autograd.grad(_loss(hseq, hsel, w.to(dtype), wsel.to(dtype)), leaves, retain_graph=i + 1 < len(cotangents))
        grads.append(dict(zip(("dX", "dh0", "dWg", "dbg", "dWc", "dbc"), [gs[0].transpose(0, 1)] + list(gs[1:]))))
    return hseq.detach(), grads


_REF_CACHE = {}


def cached_reference(name, t, b, seed, rps_sparse, case=None):
    """the reference of a case at (T, B), computed once per process for the dense cotangent and -- SPARSE_CASES -- the sparse one"""
    key = (name, t, b, seed, rps_sparse)
    if key not in _REF_CACHE:
        case = case if case is not None else CASES[name]
        op = make_operands(case, t, b, seed)
        cots = [(op["w"], op["wsel"])]
        if rps_sparse is not None:
            keep = torch.zeros(b, dtype=torch.bool)
            keep[sparse_clips(b, case["n"], rps_sparse)] = True
            cots.append((op["w"] * keep.view(1, b, 1), op["wsel"] * keep.view(b, 1)))
        hseq, grads = reference(case, op, cots)
        _REF_CACHE[key] = (op, cots, hseq, grads)
    return _REF_CACHE[key]


# ---- the layer under test -------------------------------------------------------------------------------------------------------
def run_layer(case, op, w, wsel, device, need_dx=True):
    """ops.dcgru_layer forward + backward on `device` -> (hseq, gradients, the function that repeats it).  need_dx=False: x carries no
    requires_grad and no dX comes back -- a first layer (the spectral form takes input widths other than 64 only without dX)"""
    import ctypes
    from eeg_gnn_ssl_amd import _lib, ops
    n, h, m = case["n"], case["h"], hops(case)
    t, b = w.shape[:2]
    sup = [s.to(device) for s in op["sup"]]
    p, p_batched = ops.hop_polys(sup, case["k"], b)
    assert p_batched == (1 if case.get("sup", "per_clip") == "per_clip" else 0)           # per-clip graphs: the general path
    basis = None
    if case.get("sup") == "symmetric":                                                    # the layer is handed the eigenbasis: the spectral form where it applies
        basis = ops.shared_spectral_basis(sup, case["k"])
        assert basis is not None, "the scaled Laplacian of an undirected graph is symmetric"
    if case["bm"]:
        dims = _lib.LayerDims(t, b, n, h, case["fin"], m, 0, 1)
        assert _lib.get_lib().query("eeg_dcrnn_batch_major_ok", ctypes.byref(dims)) == 2
    xb = op["xb"].to(device) if case["bm"] else op["xb"].transpose(0, 1).contiguous().to(device)      # bm: (B,T,N,F) storage
    par = {q: op[q].to(device) for q in ("wg", "bg", "wc", "bc")}
    h0 = op["h0"].to(device) if op["h0"] is not None else None
    lengths = op["lengths"].to(device) if op["lengths"] is not None else None
    wd, wseld = w.to(device), wsel.to(device)

    def run():
        x = xb.detach().requires_grad_(need_dx)
        q = {k: v.detach().requires_grad_(True) for k, v in par.items()}
        h0d = h0.detach().requires_grad_(True) if h0 is not None else None
        if basis is None:
            hseq, hsel = ops.dcgru_layer(x.transpose(0, 1) if case["bm"] else x, h0d, p, p_batched, q["wg"], q["bg"], q["wc"], q["bc"],
                                         n, h, m, case["act"], lengths)
        else:
            out = ops.dcgru_layer_ex(x, 0, h0d, p, p_batched, q["wg"], q["bg"], q["wc"], q["bc"], n, h, m, case["act"], lengths, basis=basis)
            hseq, hsel = out.hseq, out.hsel
        _loss(hseq, hsel if lengths is not None else None, wd, wseld).backward()
        run.hsel = hsel.detach() if lengths is not None else None                         # (the state at each clip's last step, as returned)
        grads = dict(dWg=q["wg"].grad, dbg=q["bg"].grad, dWc=q["wc"].grad, dbc=q["bc"].grad)
        if need_dx:
            grads["dX"] = x.grad.transpose(0, 1) if case["bm"] else x.grad
        if h0d is not None:
            grads["dh0"] = h0d.grad
        return hseq.detach(), grads

    def forward_only():
        """the same layer under torch.no_grad(): nothing is saved for a backward (Rs == nullptr in the recurrent kernel)"""
        with torch.no_grad():
            if basis is None:
                return ops.dcgru_layer(xb.transpose(0, 1) if case["bm"] else xb, h0, p, p_batched, par["wg"], par["bg"], par["wc"], par["bc"],
                                       n, h, m, case["act"], lengths)[0]
            return ops.dcgru_layer_ex(xb, 0, h0, p, p_batched, par["wg"], par["bg"], par["wc"], par["bc"], n, h, m, case["act"], lengths, basis=basis).hseq
    run.forward_only = forward_only
    return run


def assert_roles(ran, expect, what, exact=True):
    """the recorder's {role: {symbol: launches}} of ONE forward + backward against a case's expectation: each expected role went out
    once, as the expected kernel, and no other h-part role ran.  exact=False (the emulator's small row counts, where the split NN
    kernels are planned with narrower column blocks): the split kernels are compared by name, the quad kernels still by instance"""
    def norm(sym):
        return sym if exact or is_quad(sym) else sym.split("<")[0]
    got = {role: {norm(s): c for s, c in ran.get(role, {}).items()} for role in ROLES if role in ran or role in expect}
    want = {role: {norm(sym): 1} for role, sym in expect.items()}
    assert got == want, f"{what}: kernels that ran {got}, expected {want}"


def check_case(name, device, rows_min, cus=None, exe=None, sparse=False, seed=0, report=None, exact=True, dims=None, case=None,
               grad_tol=GRAD_TOL, need_dx=True):
    """One case: the layer on `device` against the float64 reference (hseq under assert_close, every gradient under
    assert_close_scaled(tol=5e-5)), after the proof that the expected kernels took its GEMMs.  sparse: the cotangent lives on three clips
    (first, last, and the one across the first row-split boundary of the case's quad TN kernel, read from the plan driver `exe`), so
    that a row dropped, doubled or misplaced at a split or tile edge is measured against a few hundred rows' worth of gradient.
    case: a case of another table in this format (tests/split_gemm_suite.py), at the `dims` it names; grad_tol: its gradient bound;
    need_dx=False: the layer is not asked for dX (run_layer)."""
    case = case if case is not None else CASES[name]
    t, b, r = dims if dims is not None else case_dims(case, rows_min)
    rps = None
    if exe is not None and name in SPARSE_CASES:  # (the reference of such a case carries both cotangents: one float64 forward)
        roles, splits = planned(exe, [(case["h"], hops(case), case["fin"], r, case["bm"], cus)])[0]
        rps = splits["gemm_tn_x"] if is_quad(roles["gemm_tn_x"]) else splits["gemm_tn_hg"]
        assert rps < r, (name, rps, r)
    assert rps is not None or not sparse
    op, cots, ref_hseq, ref_grads = cached_reference(name, t, b, seed, rps, case)
    which = 1 if sparse else 0
    run = run_layer(case, op, *cots[which], device, need_dx=need_dx)
    run()                                                                                 # (first call: allocations)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=run()))
    hseq, grads = out["res"]
    what = f"{name}{' (sparse)' if sparse else ''} T={t} B={b} R={r}"
    assert_roles(ran, case["expect"], what, exact)
    errs = {"hseq": ps.rel_err(hseq.cpu().numpy(), ref_hseq.numpy())}
    for k, g in grads.items():
        ref = ref_grads[which][k].numpy()
        errs[k] = float(abs(g.detach().cpu().double().numpy() - ref).max() / max(abs(ref).max(), 1e-6))
    print(f"quad-gemm {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"quad-gemm {what} ran: " + "; ".join(f"{role} = {sym}" for role in ROLES for sym in ran.get(role, {})))
    if report is not None:
        report[what] = errs
    ps.assert_close(hseq.cpu().numpy(), ref_hseq.numpy(), f"{what}: hseq")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[which][k].numpy(), f"{what}: {k}", tol=grad_tol)
    if sparse and need_dx:                        # clips without a cotangent: not one bit of gradient reaches their inputs
        keep = sparse_clips(b, case["n"], rps)
        rest = [i for i in range(b) if i not in keep]
        assert not grads["dX"][:, rest].any(), f"{what}: dX of a clip without a cotangent is not zero"
    return errs, ran
