"""The split GEMMs of csrc/kernels_gemm.h (gemm_nn_dma_kernel, gemm_nn_kernel, gemm_tn_dma_kernel, gemm_tn_kernel) at every template
instance a product build can reach.  They take every hoisted GEMM below 256 rows per CU, every role the whole-block kernels do not
cover, the decoder's projection and the stand-alone dconv operator -- and dconv reaches all of their instances: one diffusion plus
one GEMM with free (M, F, B*N, O).  So most cases here are ONE dconv call, forward and backward, against a float64 evaluation of the
same operation written out in closed form; three single-layer cases add what dconv cannot reach (the row map of a batch-major
input, ycol0 / ldy of the candidate problem), three more the opt-in bf16 split of kernels_gemm_bf.h.  The event recorder proves
which kernel took each GEMM (`parity_suite.kernels_run`); the plan driver of tests/emu says, without a GPU, which instances are
reachable at all, and the tables must name exactly that set.  Run by tests/test_split_gemm.py on the MI355X library and, at small
row counts and under the dev knobs, by tests/test_emu_parity.py on the emulator."""
import subprocess

import numpy as np
import torch

import parity_suite as ps
import quad_gemm_suite as qg
from quad_gemm_suite import nn_dma, nn_staged, tn_dma, tn_staged

GRAD_TOL = qg.GRAD_TOL                # dW, db, dX of a dconv call and every gradient of a layer case (assert_close_scaled)
TABLE_CUS = 256                       # the CU count the tables' plans are stated for (MI355X); below the quad threshold nothing depends on it
KNOB_KEYS = (0, 1, 2, 4, 14, 15, 16, 19)      # include/eeg_dcrnn_dev.h keys behind the eight knob fields of a driver line, in order


def nn_bf3(ntb):
    return f"gemm_nn_bf3_kernel<{ntb}>"


def knob_string(knobs):
    """{dev key: value} -> the KNOBS fields of a driver line"""
    assert set(knobs) <= set(KNOB_KEYS), knobs
    return " ".join(str(knobs.get(k, 0)) for k in KNOB_KEYS)


# ---- the dconv cases --------------------------------------------------------------------------------------------------------------
# (M hop matrices counting the identity, F columns of x, N nodes, B clips, O output columns, p_batched).  R = B*N rows.  expect: the
# symbols of the forward NN (M segments of F, O/16 column tiles), the input-gradient NN (one segment of O, ceil(M*F/16) tiles, ldc =
# M*F) and the weight-gradient TN (K = M*F, O columns); tn: what the case is about in the TN plan (remap: the XCD placement, empty:
# planned splits beyond the last row).  Every expect and every tn field is the plan driver's answer for the case at 256 CUs
# (split_gemm_suite.dconv_planned; tests/test_split_gemm.py test_case_table_plans_what_it_names holds the table against it).
DCONV_CASES = {
    # one clip, no hop matrix, 16 columns: R < 128, a single 16-column tile, the register-staged kernels on both sides
    "r19_m1_o16": dict(dims=(1, 4, 19, 1, 16, 0),
                       expect=dict(fwd=nn_staged(2, 4), dx=nn_dma(2, 16), tn=tn_staged(1)), tn=dict(remap=0)),
    # M*F = 60: the last column tile of dX is wider than ldc, K of the TN is no multiple of 64 and its one k-block straddles all segments
    "r57_m3_f20": dict(dims=(3, 20, 19, 3, 48, 1),
                       expect=dict(fwd=nn_dma(2, 20), dx=nn_dma(2, 16), tn=tn_dma(2, 32)), tn=dict(remap=0)),
    # seven segments in one launch; 19 row splits padded to 24: five empty ones, with the placement; R % 32 = 13, a short last split
    "r2413_m7": dict(dims=(7, 16, 19, 127, 64, 1),
                     expect=dict(fwd=nn_dma(2, 16), dx=nn_dma(2, 16), tn=tn_dma(2, 32)), tn=dict(remap=1, empty=5)),
    # five row splits (fewer than 8: no placement), the last one short and R % 32 = 19; K = 72
    "r627_o112": dict(dims=(2, 36, 19, 33, 112, 1),
                      expect=dict(fwd=nn_staged(2, 4), dx=nn_dma(2, 16), tn=tn_dma(4, 32)), tn=dict(remap=0)),
    # 11 column tiles through column blocks of 4 (three blocks, the last one partial) in the staged NN; the 192-column TN tile without placement
    "r760_o176": dict(dims=(2, 68, 19, 40, 176, 0),
                      expect=dict(fwd=nn_staged(2, 4), dx=nn_dma(2, 16), tn=tn_dma(6, 16)), tn=dict(remap=0)),
    # from here on R = 20 368 (R % 128 = 16: a partial last 128-row tile while several column blocks are in flight)
    # the x-part shape of the standard first layer: 12 tiles in one block of the 20-deep kernel; dX: 13 tiles in blocks of 8
    "w6_f100": dict(dims=(2, 100, 19, 1072, 192, 1),
                    expect=dict(fwd=nn_dma(6, 20), dx=nn_dma(4, 16), tn=tn_dma(6, 16)), tn=dict(remap=1)),
    # 11 of 12 tiles: a partial column block at NCTW = 6; dX: 19 tiles (M*F = 300) in blocks of 10
    "w6_o176": dict(dims=(3, 100, 19, 1072, 176, 1),
                    expect=dict(fwd=nn_dma(6, 20), dx=nn_dma(5, 16), tn=tn_dma(6, 16)), tn=dict(remap=1)),
    # 9 tiles in one block of 10; a shared hop matrix at full size
    "w5_f16": dict(dims=(5, 16, 19, 1072, 144, 0),
                   expect=dict(fwd=nn_dma(5, 16), dx=nn_dma(4, 16), tn=tn_dma(6, 16)), tn=dict(remap=1)),
    # 7 of 8 tiles: a partial column block at NCTW = 4, 20-deep
    "w4_f100": dict(dims=(2, 100, 19, 1072, 112, 1),
                    expect=dict(fwd=nn_dma(4, 20), dx=nn_dma(4, 16), tn=tn_dma(4, 32)), tn=dict(remap=1)),
    # 32 nodes (R = 20 384); 5 of 8 tiles, 16-deep; K = 48: one k-block, 160 row splits without placement
    "w4_f16_n32": dict(dims=(3, 16, 32, 637, 80, 1),
                       expect=dict(fwd=nn_dma(4, 16), dx=nn_dma(2, 16), tn=tn_dma(4, 32)), tn=dict(remap=0)),
    "w6_f16_n32": dict(dims=(3, 16, 32, 637, 192, 0),
                       expect=dict(fwd=nn_dma(6, 16), dx=nn_dma(2, 16), tn=tn_dma(6, 16)), tn=dict(remap=0)),
    # F = 36 has no LDS-DMA kernel: the staged NN with the wide column block (5 of 12 tiles)
    "w6_staged": dict(dims=(3, 36, 19, 1072, 80, 1),
                      expect=dict(fwd=nn_staged(6, 4), dx=nn_dma(4, 16), tn=tn_dma(4, 32)), tn=dict(remap=1)),
    # R = 10 127: 22 column tiles of dX (M*F = 340, the last tile 4 columns wide) reach the wide block from half the rows; 32 columns:
    # the staged TN with 64 row splits, R % 32 = 15
    "dx22_o32": dict(dims=(5, 68, 19, 533, 32, 1),
                     expect=dict(fwd=nn_staged(2, 4), dx=nn_dma(6, 16), tn=tn_staged(1)), tn=dict(remap=0)),
}
# run again with a cotangent on a few clips only: one case per width of the DMA TN kernel, the first with empty trailing splits
DCONV_SPARSE_CASES = ("r2413_m7", "w4_f100", "w6_o176")

# ---- instances that only a dev build reaches (knobs 0, 1 and 14), as dconv calls the emulator can afford ------------------------------
# name -> (dims, {dev key: value}, expect).  The column block of 6 tiles of the staged NN kernel with 16-, 20- or 32-deep chunks
# needs knob 0 AND more than 20 352 rows: no emulator case and, the MI355X suite loading the product library, no GPU case either.
KNOB_CASES = {
    "nn_staged_kc32": ((2, 32, 19, 9, 48, 1), {0: 1}, dict(fwd=nn_staged(2, 32), dx=nn_staged(2, 16), tn=tn_dma(2, 32))),
    "nn_staged_kc20": ((3, 20, 19, 7, 80, 1), {0: 1}, dict(fwd=nn_staged(2, 20), dx=nn_staged(2, 20), tn=tn_dma(4, 32))),
    "nn_staged_kc16": ((2, 16, 19, 16, 160, 0), {0: 1}, dict(fwd=nn_staged(2, 16), dx=nn_staged(2, 32), tn=tn_dma(6, 16))),
    "tn_staged_2": ((3, 20, 19, 9, 64, 1), {1: 1}, dict(fwd=nn_dma(2, 20), dx=nn_dma(2, 16), tn=tn_staged(2))),
    "tn_staged_4": ((2, 36, 19, 16, 112, 1), {1: 1}, dict(fwd=nn_staged(2, 4), dx=nn_dma(2, 16), tn=tn_staged(4))),
    "tn_staged_6": ((2, 68, 19, 13, 176, 0), {1: 1}, dict(fwd=nn_staged(2, 4), dx=nn_dma(2, 16), tn=tn_staged(6))),
    "tn_wide_2": ((3, 20, 19, 9, 64, 1), {14: 48}, dict(fwd=nn_dma(2, 20), dx=nn_dma(2, 16), tn=tn_dma(2, 32, 4))),
    "tn_wide_4": ((2, 100, 19, 16, 112, 1), {14: 48}, dict(fwd=nn_dma(2, 20), dx=nn_dma(2, 16), tn=tn_dma(4, 32, 4))),
    "tn_wide_6": ((5, 16, 19, 13, 144, 0), {14: 48}, dict(fwd=nn_dma(2, 16), dx=nn_dma(2, 16), tn=tn_dma(6, 16, 4))),
}
KNOB_ONLY_NOT_RUN = {nn_staged(6, 32), nn_staged(6, 20), nn_staged(6, 16)}

# ---- single-layer cases: what dconv cannot reach --------------------------------------------------------------------------------
# quad_gemm_suite's case format, run by its check_case at T = 4, B = 268 (20 368 rows: the wide column blocks, far below the quad
# kernels' 65 536).  expect: quad_gemm_suite.planned at 256 CUs, written out.
LAYER_DIMS = (4, 268, 4 * 268 * 19)
LAYER_CASES = {
    # the standard first layer, batch-major: the x-part NN and TN read x through the row map; the gate problem is the 128-column TN,
    # the candidate the 64-column one with ycol0 = 128 in rows of ldy = 192
    "bm_f100": dict(h=64, filt="laplacian", k=2, fin=100, bm=True, n=19, rows=(128, 16), act="tanh", h0=False, lengths=False,
                    expect={"gemm_nn_xw": nn_dma(6, 20), "gemm_nn_dx": nn_dma(5, 16), "gemm_tn_x": tn_dma(6, 16),
                            "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
    # five planes of 16 through the row map, 16-deep
    "bm_f16_m5": dict(h=64, filt="dual_random_walk", k=2, fin=16, bm=True, n=19, rows=(128, 16), act="relu", h0=True, lengths=True,
                      expect={"gemm_nn_xw": nn_dma(6, 16), "gemm_nn_dx": nn_dma(4, 16), "gemm_tn_x": tn_dma(6, 16),
                              "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
    # 32 units, time-major, Fin = 36: the staged x-part NN; the candidate problem (32 columns at ycol0 = 64, ldy = 96) on the staged TN
    "tm_h32_f36": dict(h=32, filt="laplacian", k=2, fin=36, bm=False, n=19, rows=(128, 16), act="tanh", h0=True, lengths=False,
                       expect={"gemm_nn_xw": nn_staged(6, 4), "gemm_nn_dx": nn_dma(4, 16), "gemm_tn_x": tn_dma(4, 32),
                               "gemm_tn_hg": tn_dma(2, 32), "gemm_tn_hc": tn_staged(1)}),
}

# ---- the opt-in bf16 split (ops.set_gemm_mode(1)): small single-layer cases, 64 units -------------------------------------------------
# gemm_nn_bf3_kernel<12> takes the x-part (12 column tiles); dX by ceil(M*Fin/16): 20 tiles -> <10>, 8 -> <8>, 19 -> the fp32 kernel
BF3_DIMS = (4, 2, 4 * 2 * 19)
BF3_CASES = {
    "bf3_dx10": dict(h=64, filt="dual_random_walk", k=2, fin=64, bm=False, n=19, rows=(8, 0), act="tanh", h0=False, lengths=False,
                     expect={"gemm_nn_xw": nn_bf3(12), "gemm_nn_dx": nn_bf3(10), "gemm_tn_x": tn_dma(6, 16),
                             "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
    "bf3_dx8": dict(h=64, filt="laplacian", k=1, fin=64, bm=False, n=19, rows=(8, 0), act="relu", h0=True, lengths=True,
                    expect={"gemm_nn_xw": nn_bf3(12), "gemm_nn_dx": nn_bf3(8), "gemm_tn_x": tn_dma(6, 16),
                            "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
    "bf3_dx19_fp32": dict(h=64, filt="laplacian", k=2, fin=100, bm=True, n=19, rows=(8, 0), act="tanh", h0=False, lengths=False,
                          expect={"gemm_nn_xw": nn_bf3(12), "gemm_nn_dx": nn_dma(2, 16), "gemm_tn_x": tn_dma(6, 16),
                                  "gemm_tn_hg": tn_dma(4, 32), "gemm_tn_hc": tn_dma(2, 32)}),
}


# ---- the plan driver's answers ----------------------------------------------------------------------------------------------------
def drive(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def nn_symbol(line):
    """a driver nn line -> symbol, or None where the plan carries an error (a shape the caller never launches)"""
    f = line.split()
    if f[-1] != "0":
        return None
    kind, t1, t2 = int(f[0]), int(f[1]), int(f[2])
    return [qg.NNR, nn_dma(t1, t2), nn_staged(t1, t2), nn_bf3(t1)][kind]


def tn_symbol(line, row_map=False):
    f = line.split()
    if f[-1] != "0":
        return None
    return qg._tn_symbol(line, row_map)


def dconv_calls(m, f, n, b, o, cus=TABLE_CUS, knobs=qg.NO_KNOBS):
    """the three GEMMs of eeg_dcrnn_dconv_fwd / eeg_dcrnn_dconv_bwd (csrc/api.cpp) as driver lines"""
    r = b * n
    return [f"nn {m} {f} {r} {o // 16} {o} {o} 0 0 0 {cus} {knobs}",
            f"nn 1 {o} {r} {(m * f + 15) // 16} {m * f} {m * f} 0 0 0 {cus} {knobs}",
            f"tn {m} {f} {r} {o} 0 0 {cus} {knobs}"]


def projection_calls(h, dout, r, cus=TABLE_CUS, knobs=qg.NO_KNOBS):
    """the decoder's projection, its input gradient and its weight gradient (eeg_dcrnn_decoder_fwd / _bwd)"""
    return [f"nn 1 {h} {r} {(dout + 15) // 16} {dout} {dout} 0 0 0 {cus} {knobs}",
            f"nn 1 {dout} {r} {(h + 15) // 16} {h} {h} 0 0 0 {cus} {knobs}",
            f"tn 1 {dout} {r} {h} 0 0 {cus} {knobs}"]


def dconv_planned(exe, dims_list, cus=TABLE_CUS, knobs=qg.NO_KNOBS):
    """dims_list of (M, F, N, B, O[, p_batched]) -> per entry ({fwd, dx, tn: symbol}, facts): facts holds what the edge assertions of
    tests/test_split_gemm.py read -- NCTW, column tiles and column blocks of the two NN plans, nsplit, rps, k-blocks and remap of the TN"""
    lines = [ln for d in dims_list for ln in dconv_calls(*d[:5], cus=cus, knobs=knobs)]
    out = drive(exe, lines)
    res = []
    for i, d in enumerate(dims_list):
        m, f, n, b, o = d[:5]
        fwd, dx, tn = (ln.split() for ln in out[3 * i:3 * i + 3])
        assert fwd[-1] == dx[-1] == tn[-1] == "0", (d, out[3 * i:3 * i + 3])
        facts = dict(r=b * n, fwd_nctw=int(fwd[1]), fwd_nct=o // 16, fwd_gy=int(fwd[5]), dx_nctw=int(dx[1]), dx_nct=(m * f + 15) // 16, dx_gy=int(dx[5]),
                     nsplit=int(tn[4]), rps=int(tn[5]), tn_gx=int(tn[6]), remap=int(tn[10]))
        res.append((dict(fwd=nn_symbol(out[3 * i]), dx=nn_symbol(out[3 * i + 1]), tn=tn_symbol(out[3 * i + 2])), facts))
    return res


def bf3_planned(exe, case, r, cus=TABLE_CUS):
    """roles of a layer under the bf16 split: the two NN calls carry the tile counts of the term packs (kernels_gemm_bf.h make_pack3)"""
    h, m, fin = case["h"], qg.hops(case), case["fin"]
    roles, _ = qg.planned(exe, [(h, m, fin, r, case["bm"], cus)])[0]
    calls = qg.layer_calls(h, m, fin, r, case["bm"], cus)[:2]
    lines = []
    for ln, nct in zip(calls, (3 * h // 16, (m * fin + 15) // 16)):
        f = ln.split()
        f[9] = str(nct)                                                                   # bf3_nct
        lines.append(" ".join(f))
    out = drive(exe, lines)
    roles["gemm_nn_xw"], roles["gemm_nn_dx"] = nn_symbol(out[0]), nn_symbol(out[1])
    return roles


SWEEP_ROWS = (19, 127, 128, 627, 896, 1024, 2432, 10112, 10127, 20352, 20368, 45600, 65535, 65536, 291840)
HOP_COUNTS = (1, 2, 3, 4, 5, 7)


def reachable_instances(exe, knobs=qg.NO_KNOBS, widths=range(4, 520, 4), cus=TABLE_CUS):
    """every split instance some supported call is planned with: layers of 16 / 32 / 64 units, every supported hop count, input widths
    4..516, both layouts; dconv with O = 16..192; the decoder's projection with Dout = 4..256; 19 to 291 840 rows.  Plans with an error
    (a batch-major input that the kernel left cannot read: Python hands in a time-major copy instead) launch nothing."""
    lines = []
    for r in SWEEP_ROWS:
        for m in HOP_COUNTS:
            for fin in widths:
                for h in (16, 32, 64):
                    for bm in (False, True):
                        lines += qg.layer_calls(h, m, fin, r, bm, cus, knobs)[:5]
                for o in range(16, 208, 16):
                    lines += dconv_calls(m, fin, 1, r, o, cus, knobs)
        for h in (16, 32, 64):
            for dout in range(4, 260, 4):
                lines += projection_calls(h, dout, r, cus, knobs)
    plans = set()
    for ln, o in zip(lines, drive(exe, lines)):
        f = o.split()
        plans.add((ln[:2], int(f[0]), int(f[1]), int(f[2]), f[-1]))
    found = set()
    for call, kind, t1, t2, error in plans:
        if error != "0" or kind == 0:                                                     # (kind 0: the whole-block kernels, tests/quad_gemm_suite.py)
            continue
        found.add([None, nn_dma(t1, t2), nn_staged(t1, t2), nn_bf3(t1)][kind] if call == "nn" else
                  [None, tn_dma(t1, t2), tn_dma(t1, t2, 4), tn_staged(t1)][kind])
    return found


def named_instances():
    """the split symbols the product tables name"""
    syms = {s for c in DCONV_CASES.values() for s in c["expect"].values()}
    syms |= {s for c in LAYER_CASES.values() for s in c["expect"].values()}
    return syms


# ---- operands, the float64 reference ----------------------------------------------------------------------------------------------
def make_dconv_operands(dims, seed=0):
    m, f, n, b, o, pb = dims
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(b if pb else 1, m - 1, n, n, generator=g) + 0.05
    p = p / p.sum(-1, keepdim=True)                                                       # row-stochastic, one set per clip (pb) or one for all
    k = m * f
    return dict(x=torch.randn(b, n, f, generator=g), p=p, w=torch.randn(k, o, generator=g) / k ** 0.5, bias=0.1 * torch.randn(o, generator=g),
                dout=torch.randn(b, n, o, generator=g))


def dconv_sparse_clips(b, n, rps):
    """clip 0, the last clip, the clip that holds row rps (the first row of the second split) and the clip that holds the first row of
    the last split that has rows (rows are clip * n + node)"""
    r = b * n
    last = (-(-r // rps) - 1) * rps
    return sorted({0, b - 1, rps // n, last // n})


def dconv_reference(dims, op, douts, dtype=torch.float64):
    """Z[b,n,f*M+m] = (P_m x)[b,n,f] with P_0 = I;  Y = Z W + bias;  per cotangent dY: dX = sum_m P_m^T (dY W^T)_m, dW = Z^T dY,
    db = colsum dY -- written out, no autograd.  (dtype: the same evaluation in fp32 is the yardstick of
    profiles/split_gemm_parity.txt, not a reference)"""
    m, f, n, b, o, pb = dims
    x, p, w, bias = (op[q].to(dtype) for q in ("x", "p", "w", "bias"))
    p = p.expand(b, m - 1, n, n)
    planes = [x] + [torch.bmm(p[:, j], x) for j in range(m - 1)]
    z = torch.stack(planes, dim=-1).reshape(b * n, f * m)
    y = (z @ w + bias).reshape(b, n, o)
    grads = []
    for dout in douts:
        dy = dout.to(dtype).reshape(b * n, o)
        dz = (dy @ w.t()).reshape(b, n, f, m)
        dx = dz[..., 0].clone()
        for j in range(m - 1):
            dx += torch.bmm(p[:, j].transpose(1, 2), dz[..., j + 1])
        grads.append(dict(dX=dx, dW=z.t() @ dy, db=dy.sum(0)))
    return y, grads


_REF_CACHE = {}


def cached_dconv_reference(dims, seed, rps_sparse):
    key = (dims, seed, rps_sparse)
    if key not in _REF_CACHE:
        op = make_dconv_operands(dims, seed)
        douts = [op["dout"]]
        if rps_sparse is not None:
            keep = torch.zeros(dims[3], dtype=torch.bool)
            keep[dconv_sparse_clips(dims[3], dims[2], rps_sparse)] = True
            douts.append(op["dout"] * keep.view(-1, 1, 1))
        y, grads = dconv_reference(dims, op, douts)
        _REF_CACHE[key] = (op, douts, y, grads)
    return _REF_CACHE[key]


# ---- the operator under test ------------------------------------------------------------------------------------------------------
def run_dconv(dims, op, dout, device):
    """torch.ops.eeg_dcrnn.dconv and its autograd on `device` -> the function that runs it once: (Y, {dX, dW, db})"""
    import eeg_gnn_ssl_amd  # noqa: F401  (registers the operators)
    pb = dims[5]
    x, p, w, bias, dy = (t.to(device) for t in (op["x"], op["p"], op["w"], op["bias"], dout))

    def run():
        xs, ws, bs = (t.detach().requires_grad_(True) for t in (x, w, bias))
        y = torch.ops.eeg_dcrnn.dconv(xs, p, pb, ws, bs)
        y.backward(dy)
        return y.detach(), dict(dX=xs.grad, dW=ws.grad, db=bs.grad)
    return run


def assert_dconv_kernels(ran, expect, what, exact=True):
    """the recorder's {role: {symbol: launches}} of ONE dconv forward + backward: under gemm_nn the forward and the input-gradient symbol,
    under gemm_tn the weight-gradient symbol, once each (twice where forward and input gradient share an instance), nothing else"""
    def norm(sym):
        return sym if exact else sym.split("<")[0]
    want_nn = {}
    for s in (expect["fwd"], expect["dx"]):
        want_nn[norm(s)] = want_nn.get(norm(s), 0) + 1
    got = {}
    for role in ("gemm_nn", "gemm_tn"):
        got[role] = {}
        for s, c in ran.get(role, {}).items():
            got[role][norm(s)] = got[role].get(norm(s), 0) + c
    want = {"gemm_nn": want_nn, "gemm_tn": {norm(expect["tn"]): 1}}
    assert got == want, f"{what}: kernels that ran {got}, expected {want}"
    others = [r for r in ran if r.startswith("gemm_") and r not in want]
    assert not others, f"{what}: unexpected GEMM roles {others}"


def _scaled_err(got, ref):
    ref = ref.numpy()
    return float(np.abs(got.detach().cpu().double().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6))


def check_dconv(name, device, exe, cus, dims=None, expect=None, sparse=False, seed=0, report=None, exact=True, knobs=None):
    """One dconv case on `device`: the recorder's kernels against the case's expectation AND against the plan driver's answer for this
    call at `cus` CUs, then Y (assert_close) and dX, dW, db (assert_close_scaled, 5e-5) against the float64 reference.  sparse: the
    cotangent lives on the clips of dconv_sparse_clips, and dX of every other clip must be exactly zero.  dims / expect / knobs: the
    emulator's smaller clip count and the dev-knob cases"""
    case = DCONV_CASES.get(name)
    dims = dims if dims is not None else case["dims"]
    expect = expect if expect is not None else case["expect"]
    m, f, n, b, o, pb = dims
    planned, facts = dconv_planned(exe, [dims], cus=cus, knobs=knob_string(knobs or {}))[0]
    rps = facts["rps"] if sparse else None
    op, douts, ref_y, ref_grads = cached_dconv_reference(dims, seed, rps)
    which = 1 if sparse else 0
    run = run_dconv(dims, op, douts[which], device)
    run()                                                                                 # (first call: allocations)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=run()))
    y, grads = out["res"]
    what = f"{name}{' (sparse)' if sparse else ''} M={m} F={f} N={n} B={b} O={o} R={b * n}"
    assert_dconv_kernels(ran, expect, what, exact)
    assert_dconv_kernels(ran, planned, what + " (plan driver)", True)
    errs = {"Y": ps.rel_err(y.cpu().numpy(), ref_y.numpy())}
    errs.update({k: _scaled_err(g, ref_grads[which][k]) for k, g in grads.items()})
    print(f"split-gemm {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"split-gemm {what} ran: " + "; ".join(f"{role} = {sym} x{c}" for role in ("gemm_nn", "gemm_tn") for sym, c in ran.get(role, {}).items()))
    if report is not None:
        report[what] = (errs, ran)
    ps.assert_close(y.cpu().numpy(), ref_y.numpy(), f"{what}: Y")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[which][k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
    if sparse:                                    # clips without a cotangent: not one bit of gradient reaches their inputs
        keep = dconv_sparse_clips(b, n, rps)
        assert len(keep) >= 3 and rps < b * n, (what, keep, rps)
        rest = [i for i in range(b) if i not in keep]
        assert not grads["dX"][rest].any(), f"{what}: dX of a clip without a cotangent is not zero"
        assert grads["dX"][keep].abs().sum() > 0
    return errs, ran


def emu_dims(dims):
    """a case at a row count the emulator can afford (it runs one lane at a time): the cases up to 2 432 rows as they are (r2413_m7
    with its 24 placed row splits, five of them empty), the others at 16 clips of 19 nodes (304 rows: two whole 128-row tiles and a
    partial one, three TN row splits) or 9 of 32"""
    m, f, n, b, o, pb = dims
    return dims if b * n <= 2432 else (m, f, n, 304 // n, o, pb)


def fp32_yardstick(name):
    """the float64 reference of a dconv or layer case of these tables evaluated in fp32 on the host, against the reference: the error
    level of a correct fp32 evaluation at the case's size (profiles/split_gemm_parity.txt; not asserted anywhere)"""
    if name in DCONV_CASES:
        dims = DCONV_CASES[name]["dims"]
        op, douts, ref_y, ref_grads = cached_dconv_reference(dims, 0, None)
        y, grads = dconv_reference(dims, op, douts[:1], dtype=torch.float32)
        errs = {"Y": ps.rel_err(y.numpy(), ref_y.numpy())}
        errs.update({k: _scaled_err(g, ref_grads[0][k]) for k, g in grads[0].items()})
        return errs
    case, (t, b, _) = (LAYER_CASES[name], LAYER_DIMS) if name in LAYER_CASES else (BF3_CASES[name], BF3_DIMS)
    op, cots, ref_hseq, ref_grads = qg.cached_reference(name, t, b, 0, None, case)
    hseq, grads = qg.reference(case, op, cots[:1], dtype=torch.float32)
    errs = {"hseq": ps.rel_err(hseq.numpy(), ref_hseq.numpy())}
    errs.update({k: _scaled_err(g, ref_grads[0][k]) for k, g in grads[0].items()})
    return errs


# ---- layer cases (quad_gemm_suite.check_case on a case of these tables) ----------------------------------------------------------------
def check_layer(name, device, report=None):
    return qg.check_case(name, device, None, dims=LAYER_DIMS, case=LAYER_CASES[name], report=report)


def check_bf3_layer(name, device, report=None):
    """a BF3_CASES layer under ops.set_gemm_mode(1): the recorder proves the bf16-split kernels (and, for 19 tiles of dX, the fp32
    kernel) took the NN GEMMs; hidden sequence and gradients at the tolerances of parity_suite.check_split_bf16 (2e-5 both)"""
    from eeg_gnn_ssl_amd import ops
    prev = ops.set_gemm_mode(1)
    try:
        return qg.check_case(name, device, None, dims=BF3_DIMS, case=BF3_CASES[name], grad_tol=ps.TOL, report=report)
    finally:
        ops.set_gemm_mode(prev)
