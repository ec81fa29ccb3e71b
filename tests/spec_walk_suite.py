"""The hoisted GEMMs of the spectral form (csrc/kernels_gemm_f.h, kernels_gemm_g.h, kernels_spectral.h) where their rings, counted waits and
persistent row ranges ENGAGE.  tests/spec_plan_suite.py pins every instance, but at 12 or 15 rows per frequency: on 256 CUs every
gemm_nnf_kernel workgroup then walks one chunk (no stage is ever reused, only the n = 0 arm of the wait ladder is taken, no range crosses
a frequency), gemm_tnf_kernel walks two, gemm_nng_kernel never forms a 128-row tile and no mix grid is capped.  Here every case is ONE
DCGRU layer (`quad_gemm_suite.run_layer` with the symmetric support: ops.dcgru_layer_ex(..., basis=...)) at a row count chosen so that the
walk of each kernel -- restated below in Python from the grid, spg and rps of the plan driver's own line for the call -- visits the
states listed in REQUIRED, against `quad_gemm_suite.reference` in float64: hseq under assert_close, every gradient under
assert_close_scaled(5e-5), the forward again under no_grad bit for bit, and -- three cases -- a cotangent on three clips only, so that
one row lost or doubled at a split or chunk edge is measured against a few hundred rows and not against 10^5.

Run by tests/test_spec_walk.py (the table against the rules without a GPU; every case on the MI355X) and, at the emulator's 4 CUs, by
tests/test_emu_parity.py (TWINS).  The emulator executes a DMA when it is requested: the twins catch a wrong stage, range or boundary
index, never a wait that is too weak or a stage overwritten too early -- that is what the MI355X cases are for."""
import subprocess

import torch

import parity_suite as ps
import quad_gemm_suite as qg
import spec_plan_suite as sp

TABLE_CUS = 256                       # the CU count the table's row counts are chosen for (MI355X)
GRAD_TOL = qg.GRAD_TOL
SEED = 0
NNF_NS, NNG_NS = 3, 4                # ring depths: spec_launch.h kNnfNS, kNngStages
TNF_RC, TNG_RC, DXF_ROWS = 8, 16, 32  # rows per chunk / per workgroup: kTnfRC, kSpecTngRc, kDxfRows
NNF_ARMS = (63, 55, 52, 48, 14, 8, 7, 4, 0)          # the counts gemm_nnf_kernel has a wait for, largest first

TNF4_R4 = sp.tnf(4) + " [Fin = 100: tnf_role_r4]"     # the two roles of the one instance are walked (and required) apart
TNF4_GENERAL = sp.tnf(4) + " [general role]"


def tnf_ns(fxt):
    return 3 if fxt <= 2 else 5       # spec_launch.h tnf_ns


# ---- the states ------------------------------------------------------------------------------------------------------------------
NNF_STATES = {"ring reused (Q >= 4: steady arm 96 + PER)", "q = 0 with a next chunk (n = PER)", "q = 1 with a next chunk (n = 48 + PER)",
              "last chunk (nd = 0)", "range crosses a frequency strictly inside", "Sp % 64 != 0", "S % 16 != 0"}
NNG_STATES = {"full tile, then chunks with dma and more (burst wait)", "tile cut at a group boundary", "short last tile",
              "all three in one workgroup's range"}
TNG_STATES = {"spg > 1", "last split shorter than rps"}
DXF_STATES = {"Sp % 32 == 16", "S < Sp", "more than one workgroup"}
CAPPED = "grid capped: a second grid-stride pass"


def tnf_states(fxt):
    ns = tnf_ns(fxt)
    # FXT <= 2: NS - 1 = 2 chunks is the shortest split the rule allows at all (splits are whole 16-row units): that one is required
    short = f"a split with Q < NS - 1 = {ns - 1}" if fxt >= 3 else "a split with Q = 2 = NS - 1 (the smallest the row split allows)"
    return {"spg > 1", "last split shorter than rps", f"a split with Q >= NS + 1 = {ns + 1}", short}


REQUIRED = {
    **{sp.nnf(kq, kq == 8): NNF_STATES for kq in (13, 9, 8, 5, 2)},
    sp.nng(3): NNG_STATES | {"tail chunk (Fin = 132: 8 whole chunks + 1 piece)", "no tail chunk (Fin = 128)"},
    sp.nng(1): NNG_STATES,
    sp.tnf(1): tnf_states(1), sp.tnf(2): tnf_states(2), sp.tnf(3): tnf_states(3), TNF4_R4: tnf_states(4), TNF4_GENERAL: tnf_states(4),
    sp.tng(5): TNG_STATES, sp.tng(4): TNG_STATES | {"nkb = 2"}, sp.TNG_PAIR: TNG_STATES,
    sp.dxf(19): DXF_STATES, sp.dxf(0): DXF_STATES,
    sp.mix_mfma(0, 10): {CAPPED}, sp.mix_mfma(0, 16): {CAPPED}, sp.mix_mfma(1, 16): {CAPPED}, sp.MIX_GENERIC: {CAPPED},
    # spec_mix_in_kernel<19>: its cap (1024 workgroups) needs more than 10 240 rows at F = 100 and more below, which no case here has
    # (the full-size cfg2 test of tests/test_gpu_parity.py runs it capped at F = 100): the four widths are walked uncapped.  Open.
    sp.MIX_IN19: {"F = 100", "F = 68", "F = 36", "F = 12"},
}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# One layer: n nodes, fin features, dx (the layer is asked for dX: a layer above the first; else x carries no requires_grad, as the
# spectral form covers Fin != 64 for layer 0 only), k diffusion steps (M = k + 1; the hoisted GEMMs have K = Fin whatever M is), rows =
# the S = T*B it runs at (first: the deep walk; a second one where one row count cannot give all states: Sp = 80 is two splits of 64 and
# 16 rows).  expect: role -> symbols that MUST be recorded (format of spec_plan_suite.CASES).  Row counts are chosen for 256 CUs:
# S = 6120 = 17 * 360, Sp = 6128 (Sp % 64 = 48, Sp % 32 = 16): 96 chunks per frequency, 1824 chunks over 512 workgroups.
# Every case runs tanh: the activation is the recurrent kernels' business (tests/seq_kernel_suite.py), and at 7.4 million candidate
# elements relu puts some pre-activation within fp32 rounding of its kink.  Measured with n19_f68 under relu on the MI355X: hseq 5.5e-7,
# but dbc 1.3e-3 and dWc 2.8e-3 -- all of it one element (t 14, clip 19, node 2, unit 18) whose float64 pre-activation is -1.25e-7 and
# whose dL/dc = 0.830 is the 0.798 by which dbc[18] differed (no other column by more than 0.058); 9 elements lie within 1e-6 of zero.
# Seed 1 and the same layer under tanh gave 4e-7 everywhere.  A sign on the kink is not a property of these GEMMs.
def _case(n, fin, dx, rows, expect, k=1, h0=False, lengths=False, act="tanh", knobs=sp.NO_KNOBS):
    return dict(n=n, fin=fin, dx=dx, rows=rows, expect=expect, k=k, h=64, filt="laplacian", sup="symmetric", bm=False, h0=h0, lengths=lengths,
                act=act, knobs=knobs)


CASES = {
    "n19_f64_dx": _case(19, 64, True, (6120, 78), k=2, h0=True, lengths=True,
                        expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_f": {sp.tnf(2)}, "gemm_dx_f": {sp.dxf(19)}, "spec_mix_x": {sp.mix_mfma(0, 10)}}),
    "n19_f100": _case(19, 100, False, (6120, 78),
                      expect={"gemm_nn_xw": {sp.nnf(13)}, "gemm_tn_f": {sp.tnf(4)}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f68": _case(19, 68, False, (6120, 78),
                     expect={"gemm_nn_xw": {sp.nnf(9)}, "gemm_tn_f": {sp.tnf(3)}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f36": _case(19, 36, False, (6120, 78),
                     expect={"gemm_nn_xw": {sp.nnf(5)}, "gemm_tn_f": {sp.tnf(2)}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f12": _case(19, 12, False, (6120, 78),
                     expect={"gemm_nn_xw": {sp.nnf(2)}, "gemm_tn_f": {sp.tnf(1)}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f132": _case(19, 132, False, (6120,),
                      expect={"gemm_nn_xw": {sp.nng(3)}, "gemm_tn_x": {sp.tng(5)}, "gemm_tn_h": {sp.TNG_PAIR}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f200": _case(19, 200, False, (6120,),
                      expect={"gemm_nn_xw": {sp.nng(3)}, "gemm_tn_x": {sp.tng(4)}, "gemm_tn_h": {sp.TNG_PAIR}, "spec_mix_x": {sp.MIX_IN19}}),
    "n19_f128": _case(19, 128, False, (6120, 78),
                      expect={"gemm_nn_xw": {sp.nng(3)}, "gemm_tn_f": {sp.tnf(4)}, "spec_mix_x": {sp.mix_mfma(0, 10)}}),
    # 24 nodes: the recurrent kernels do not mix, every node mix is a pass; dX as the grouped GEMM over K = 192 and the mix back
    "n24_f64_dx": _case(24, 64, True, (6120,), h0=True,
                        expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_f": {sp.tnf(2)}, "gemm_nn_dx": {sp.nng(1)}, "spec_mix_dx": {sp.mix_mfma(1, 16)},
                                "spec_mix_x": {sp.mix_mfma(0, 16)}}),
    "n20_f64_dx": _case(20, 64, True, (1512,), lengths=True,
                        expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_f": {sp.tnf(2)}, "gemm_dx_f": {sp.dxf(0)}, "spec_mix_x": {sp.mix_mfma(0, 10)}}),
    "n18_f100": _case(18, 100, False, (1208,),
                      expect={"gemm_nn_xw": {sp.nnf(13)}, "gemm_tn_f": {sp.tnf(4)}, "spec_mix_x": {sp.MIX_GENERIC}}),
}
SPARSE_CASES = ("n19_f64_dx", "n19_f100", "n19_f132")   # also run with a cotangent on three clips only, at the first row count

# The twins at the emulator's 4 CUs (grid 8): ~110 rows per frequency already give Q >= 4.  `states`: what each must visit THERE.
_NNF_TWIN = NNF_STATES


def _twin(states, **kw):
    case = _case(**kw)
    case["states"] = states
    return case


TWINS = {
    "nnf13": _twin({sp.nnf(13): _NNF_TWIN}, n=19, fin=100, dx=False, rows=(105,),
                   expect={"gemm_nn_xw": {sp.nnf(13)}, "gemm_tn_f": {sp.tnf(4)}, "spec_mix_x": {sp.MIX_IN19}}),
    "nnf9": _twin({sp.nnf(9): _NNF_TWIN}, n=19, fin=68, dx=False, rows=(105,),
                  expect={"gemm_nn_xw": {sp.nnf(9)}, "gemm_tn_f": {sp.tnf(3)}, "spec_mix_x": {sp.MIX_IN19}}),
    "nnf8": _twin({sp.nnf(8, True): _NNF_TWIN, sp.dxf(19): DXF_STATES}, n=19, fin=64, dx=True, rows=(105,), h0=True, lengths=True, k=2,
                  expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_f": {sp.tnf(2)}, "gemm_dx_f": {sp.dxf(19)}, "spec_mix_x": {sp.mix_mfma(0, 10)}}),
    "nnf5": _twin({sp.nnf(5): _NNF_TWIN}, n=19, fin=36, dx=False, rows=(105,),
                  expect={"gemm_nn_xw": {sp.nnf(5)}, "gemm_tn_f": {sp.tnf(2)}, "spec_mix_x": {sp.MIX_IN19}}),
    "nnf2": _twin({sp.nnf(2): _NNF_TWIN}, n=19, fin=12, dx=False, rows=(105,),
                  expect={"gemm_nn_xw": {sp.nnf(2)}, "gemm_tn_f": {sp.tnf(1)}, "spec_mix_x": {sp.MIX_IN19}}),
    "nng3_tail": _twin({sp.nng(3): NNG_STATES | {"tail chunk (Fin = 132: 8 whole chunks + 1 piece)"}}, n=5, fin=132, dx=False, rows=(264,),
                       expect={"gemm_nn_xw": {sp.nng(3)}, "gemm_tn_x": {sp.tng(5)}, "gemm_tn_h": {sp.TNG_PAIR}, "spec_mix_x": {sp.MIX_GENERIC}}),
    "nng1": _twin({sp.nng(1): NNG_STATES}, n=21, fin=64, dx=True, rows=(120,),
                  expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_f": {sp.tnf(2)}, "gemm_nn_dx": {sp.nng(1)}, "spec_mix_dx": {sp.mix_mfma(1, 16)},
                          "spec_mix_x": {sp.mix_mfma(0, 16)}}),
    "tnf3_short": _twin({sp.tnf(3): tnf_states(3)}, n=2, fin=68, dx=False, rows=(78,),
                        expect={"gemm_nn_xw": {sp.nnf(9)}, "gemm_tn_f": {sp.tnf(3)}, "spec_mix_x": {sp.MIX_GENERIC}}),
    "tng_planar": _twin({sp.tng(2, True): TNG_STATES, sp.TNG_PAIR: TNG_STATES}, n=3, fin=64, dx=False, rows=(78,), knobs=(0, 1, 0),
                        expect={"gemm_nn_xw": {sp.nnf(8, True)}, "gemm_tn_x": {sp.tng(2, True)}, "gemm_tn_h": {sp.TNG_PAIR}, "spec_mix_x": {sp.mix_mfma(0, 10)}}),
}


def pick_tb(s):
    """(T, B) with T * B = s and B < 384 (below the streamed BPTT kernel's batch), the step counts tried as quad_gemm_suite.pick_rows does"""
    for t in (12, 8, 16, 13, 14, 10, 9, 11, 15, 6, 4, 5, 7, 3, 2, 1, 17, 18, 19, 20, 24, 32):
        if s % t == 0 and s // t < 384:
            return t, s // t
    raise AssertionError(f"no (T, B) with B < 384 for {s} rows")


# ---- the plan driver's lines of a layer ------------------------------------------------------------------------------------------
def _parse(line):
    """`symbol ; gx gy block lds [; symbol ; ...] [; trailing ints]` -> ([(symbol, gx, gy, block)], [trailing ints])"""
    assert not line.startswith("error"), line
    tok, launches, rest, i = line.split(" ; "), [], [], 0
    while i < len(tok):
        if sp.is_spectral(tok[i]):
            gx, gy, block, _lds = (int(v) for v in tok[i + 1].split())
            launches.append((tok[i], gx, gy, block))
            i += 2
        else:
            rest += [int(v) for v in tok[i].split()]
            i += 1
    return launches, rest


def plan_layer(exe, case, t, b, cus):
    """-> (must, may, calls): role -> set of symbols as spec_plan_suite.planned gives them for a model (a single layer always mixes its
    own input: spec_mix_x is a must), and calls = [(kind, role, launches, trailing)] with kind = the driver's op"""
    lines = sp.layer_calls(case["n"], t, b, case["fin"], case["dx"], cus, case["knobs"])
    out = subprocess.run([exe], input="".join(ln + "\n" for _, ln, _ in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    must, may, calls = {}, {}, []
    for (role, line, is_must), got in zip(lines, out):
        launches, rest = _parse(got)
        syms = [s for s, *_ in launches]
        if role == "tn":
            named = {"gemm_tn_f": syms} if len(syms) == 1 else {"gemm_tn_x": syms[:1], "gemm_tn_h": syms[1:]}
        elif role == "dx":
            named = {"gemm_dx_f": syms} if len(syms) == 1 else {"gemm_nn_dx": syms[:1], "spec_mix_dx": syms[1:]}
        else:
            named = {role: syms}
        for r, s in named.items():
            (must if is_must or r == "spec_mix_x" else may).setdefault(r, set()).update(s)
        calls.append((line.split()[0], role, launches, rest, line))
    return must, may, calls


# ---- the walks, restated ---------------------------------------------------------------------------------------------------------
def nnf_per(k):
    """1-KB requests of a 64-row chunk per wave (gemm_nnf_kernel: NPC = ceil(64 K / 256), PER = ceil(NPC / 4))"""
    return -(-(-(-64 * k // 256)) // 4)


def nnf_walk(k, s, sp_rows, g, grid):
    """gemm_nnf_kernel: workgroup bid walks chunks [bid total / grid, (bid+1) total / grid) -> (states, {Q: workgroups}, wait arms taken)"""
    cpg = -(-sp_rows // 64)
    total, per = g * cpg, nnf_per(k)
    states, qs, arms = set(), {}, set()
    for bid in range(grid):
        g0, g1 = bid * total // grid, (bid + 1) * total // grid
        q_len = g1 - g0
        qs[q_len] = qs.get(q_len, 0) + 1
        for q in range(q_len):
            nd = min(q_len - 1 - q, NNF_NS - 2)
            n = 48 * min(q, NNF_NS - 1) + per * nd
            arms.add(next(a for a in NNF_ARMS if n >= a))
            if nd == 0:
                states.add("last chunk (nd = 0)")
            elif q == 0:
                states.add("q = 0 with a next chunk (n = PER)")
            elif q == 1:
                states.add("q = 1 with a next chunk (n = 48 + PER)")
        if q_len >= 4:
            states.add("ring reused (Q >= 4: steady arm 96 + PER)")
        if q_len >= 2 and g0 // cpg != (g1 - 1) // cpg:
            states.add("range crosses a frequency strictly inside")
    if sp_rows % 64:
        states.add("Sp % 64 != 0")
    if s % 16:
        states.add("S % 16 != 0")
    return states, qs, arms


def nng_walk(f, sp_rows, g, grid):
    """gemm_nng_kernel: row tiles [bid RT / grid, (bid+1) RT / grid) of 16 rows, walked in tiles of up to 8 cut at group boundaries and at
    the range's end, nch chunks each; the chunk behind a full tile waits with `burst` where it still requests (q + NS - 1 < Q)
    -> (states, {tiles per workgroup: workgroups}, largest chunk count Q, longest tile in row tiles)"""
    nch = f // 16 + (1 if (f // 4) % 4 else 0)                 # nnq_order.h make_nnq_order(1, F).nch
    rtg = sp_rows // 16
    rt = rtg * g
    states, tiles_per, q_max, longest = set(), {}, 0, 0
    for bid in range(grid):
        rt0, rt1 = bid * rt // grid, (bid + 1) * rt // grid
        cur, tiles = rt0, []
        while cur < rt1:
            ln, to_b = min(rt1 - cur, 8), rtg - cur % rtg
            cut = to_b < ln
            tiles.append((min(ln, to_b), cut))
            cur += min(ln, to_b)
        q_len = len(tiles) * nch
        q_max, longest = max(q_max, q_len), max([longest] + [ln for ln, _ in tiles])
        tiles_per[len(tiles)] = tiles_per.get(len(tiles), 0) + 1
        here = set()
        for i, (ln, cut) in enumerate(tiles):
            if ln == 8 and (i + 1) * nch + NNG_NS - 1 < q_len:
                here.add("full tile, then chunks with dma and more (burst wait)")
            if cut and ln < 8:
                here.add("tile cut at a group boundary")
        if tiles and tiles[-1][0] < 8 and not tiles[-1][1]:
            here.add("short last tile")
        if len(here) == 3:
            here.add("all three in one workgroup's range")
        states |= here
    return states, tiles_per, q_max, longest


def split_walk(sp_rows, spg, rps, rc):
    """a row split of spec_row_split: split ls takes rows [ls rps, min((ls+1) rps, Sp)) of a frequency -> chunk counts Q per split"""
    return [(min((ls + 1) * rps, sp_rows) - ls * rps) // rc for ls in range(spg)]


def tnf_walk(fxt, sp_rows, spg, rps):
    qs, ns, states = split_walk(sp_rows, spg, rps, TNF_RC), tnf_ns(fxt), set()
    want = tnf_states(fxt)
    if spg > 1:
        states.add("spg > 1")
    if sp_rows - (spg - 1) * rps < rps:
        states.add("last split shorter than rps")
    if any(q >= ns + 1 for q in qs):
        states.add(f"a split with Q >= NS + 1 = {ns + 1}")
    if fxt >= 3 and any(q < ns - 1 for q in qs):
        states.add(f"a split with Q < NS - 1 = {ns - 1}")
    if fxt <= 2 and any(q == 2 for q in qs):
        states.add("a split with Q = 2 = NS - 1 (the smallest the row split allows)")
    assert states <= want
    return states, sorted(set(qs))


def tng_walk(sp_rows, spg, rps):
    states = set()
    if spg > 1:
        states.add("spg > 1")
    if sp_rows - (spg - 1) * rps < rps:
        states.add("last split shorter than rps")
    return states, sorted(set(split_walk(sp_rows, spg, rps, TNG_RC)))


def walk_layer(exe, case, t, b, cus):
    """-> (must, may, visited, notes): visited = {instance: set of states} of every kernel of the layer at (T, B) on `cus` CUs, notes =
    {instance: text} (Q histogram, wait arms, splits) for the record"""
    must, may, calls = plan_layer(exe, case, t, b, cus)
    s, n, fin = t * b, case["n"], case["fin"]
    sp_rows = sp.spec_rows(s)
    visited, notes = {}, {}

    def add(inst, states, note=None):
        visited.setdefault(inst, set()).update(states)
        if note:
            notes[inst] = note
    for kind, role, launches, rest, line in calls:
        if kind == "snn":
            add(*_nn_states(launches[0], fin, s, sp_rows, n))
        elif kind == "stn":
            spg_x, rps_x, spg_h, rps_h = rest[:4]
            sym, gx, gy, _ = launches[0]
            if sym.startswith("gemm_tnf_kernel"):
                fxt = int(sym.split("<")[1].rstrip(">"))
                assert gx == n * spg_x and gy == 1 and fxt == -(-fin // 32), line
                inst = sym if fxt < 4 else (TNF4_R4 if fin == 100 else TNF4_GENERAL)
                st, qs = tnf_walk(fxt, sp_rows, spg_x, rps_x)
                add(inst, st, f"spg {spg_x} rps {rps_x} Q {qs}")
            else:
                nkb = gx
                assert gy == n * spg_x and launches[1][2] == 2 * n * spg_h, line
                st, qs = tng_walk(sp_rows, spg_x, rps_x)
                add(sym, st | ({"nkb = 2"} if nkb == 2 else set()), f"nkb {nkb} spg {spg_x} rps {rps_x} Q {qs}")
                st, qs = tng_walk(sp_rows, spg_h, rps_h)
                add(launches[1][0], st, f"spg {spg_h} rps {rps_h} Q {qs}")
        elif kind == "sdx":
            sym, gx, _, _ = launches[0]
            if sym.startswith("gemm_dxf_kernel"):
                assert gx == -(-sp_rows // DXF_ROWS), line
                st = {x for x, on in (("Sp % 32 == 16", sp_rows % 32 == 16), ("S < Sp", s < sp_rows), ("more than one workgroup", gx > 1)) if on}
                add(sym, st, f"grid {gx}")
            else:
                add(*_nn_states(launches[0], 192, s, sp_rows, n))
                add(*_mix_states(launches[1], 0, n, s, sp_rows, fin))
        elif kind == "mix" and (role in must or role in may):
            f = line.split()
            to_nodes, tt, fw, node_rows = int(f[1]), int(f[3]), int(f[5]), int(f[6])
            if role in must:           # (the mixes of the 192- and 64-wide recurrent operands: walked only where they are certain to run)
                add(*_mix_states(launches[0], to_nodes, n, tt * b, node_rows or sp.spec_rows(tt * b), fw))
    return must, may, visited, notes


def _nn_states(launch, k, s, sp_rows, g):
    sym, gx, _, _ = launch
    if sym.startswith("gemm_nnf_kernel"):
        st, qs, arms = nnf_walk(k, s, sp_rows, g, gx)
        return sym, st, f"grid {gx} Q {dict(sorted(qs.items()))} PER {nnf_per(k)} wait arms {sorted(arms)}"
    st, tiles, q_max, _ = nng_walk(k, sp_rows, g, gx)
    if sym == sp.nng(3):
        st |= {"tail chunk (Fin = 132: 8 whole chunks + 1 piece)"} if k == 132 else {"no tail chunk (Fin = 128)"} if k == 128 else set()
    return sym, st, f"grid {gx} tiles per workgroup {dict(sorted(tiles.items()))} largest Q {q_max}"


def _mix_states(launch, to_nodes, n, s, sp_rows, f):
    """the grid-stride loops of kernels_spectral.h: a second pass where the work exceeds what one pass of the (capped) grid takes"""
    sym, gx, _, block = launch
    rows = sp_rows if to_nodes else s
    if sym.startswith("spec_mix_mfma_kernel"):
        second = rows * -(-f // 32) > 4 * gx                   # one (row, 32-column tile) per wave and pass
    elif sym == sp.MIX_GENERIC:
        second = rows * n * (f // 4) > 256 * gx                # one 16-byte column of one (row, node) per thread and pass
    else:
        second = rows > gx * (block // (f // 4))               # spec_mix_in / out<19>: block / F4 rows per workgroup and pass
    st = {CAPPED} if second else set()
    if sym == sp.MIX_IN19:
        st.add(f"F = {f}")
    return sym, st, f"grid {gx} {'capped' if second else 'one pass'} ({rows} rows, F = {f})"


def table_walk(exe, cases, cus):
    """-> {case: [(t, b, must, may, visited, notes) per row count]}"""
    return {name: [(*pick_tb(s), *walk_layer(exe, case, *pick_tb(s), cus)) for s in case["rows"]] for name, case in cases.items()}


def union(walks):
    out = {}
    for per_case in walks.values():
        for *_, visited, _notes in per_case:
            for inst, st in visited.items():
                out.setdefault(inst, set()).update(st)
    return out


def missing(visited, required):
    """{instance: sorted states} that `required` names and `visited` lacks"""
    return {inst: sorted(st - visited.get(inst, set())) for inst, st in required.items() if st - visited.get(inst, set())}


def case_required(exe, name, case):
    """what a case of CASES is there for: the states of REQUIRED it visits at TABLE_CUS (a twin names its own: case["states"])"""
    if "states" in case:
        return case["states"]
    seen = union({name: [(*pick_tb(s), *walk_layer(exe, case, *pick_tb(s), TABLE_CUS)) for s in case["rows"]]})
    return {inst: st & seen[inst] for inst, st in REQUIRED.items() if inst in seen and st & seen[inst]}


# ---- the reference --------------------------------------------------------------------------------------------------------------
_REF_CACHE = {}


def sparse_clips(b, rps):
    """clip 0, the last clip, and the clip that owns the first row of the second row split of a frequency (rows are t * B + b: the node
    mix does not move rows, so the rows of a frequency are the samples)"""
    return sorted({0, b - 1, rps % b})


def cached_reference(key, case, t, b, keep):
    """float64 reference of a case at (T, B) for the dense cotangent and -- keep: clips -- the sparse one, once per process"""
    key = (key, t, b, tuple(keep) if keep else None)
    if key not in _REF_CACHE:
        op = qg.make_operands(case, t, b, SEED)
        cots = [(op["w"], op["wsel"])]
        if keep:
            mask = torch.zeros(b, dtype=torch.bool)
            mask[list(keep)] = True
            cots.append((op["w"] * mask.view(1, b, 1), op["wsel"] * mask.view(b, 1)))
        hseq, grads = qg.reference(case, op, cots)
        _REF_CACHE[key] = (op, cots, hseq, grads)
    return _REF_CACHE[key]


# ---- one case -------------------------------------------------------------------------------------------------------------------
def check_case(name, device, exe, cus, sparse=False, cases=None, set_knob=None, report=None):
    """One case at each of its row counts (sparse: the first only): the walk on `cus` CUs must visit what the case is there for; the
    recorder must show the planned kernels and ops.spectral_layer_calls must advance; hseq, every gradient, the no_grad forward and --
    sparse -- the exact zeros of dX against the float64 reference."""
    from eeg_gnn_ssl_amd import ops
    cases = CASES if cases is None else cases
    case = cases[name]
    need = case_required(exe, name, case)
    walks = [(*pick_tb(s), *walk_layer(exe, case, *pick_tb(s), cus)) for s in (case["rows"][:1] if sparse else case["rows"])]
    if not sparse:
        lost = missing(union({name: walks}), need)
        assert not lost, f"{name} on {cus} CUs: states the case is there for are not visited: {lost}"
    assert case["knobs"] == sp.NO_KNOBS or set_knob is not None, "dev knobs need a development build"
    all_errs = {}
    for t, b, must, may, visited, notes in walks:
        s = t * b
        what = f"{name}{' (sparse)' if sparse else ''} T={t} B={b} S={s} Sp={sp.spec_rows(s)}"
        assert b < 384 and must == {r: set(v) for r, v in case["expect"].items()}, (what, must)
        keep = None
        if sparse or name in SPARSE_CASES and s == case["rows"][0]:      # (the reference of such a case carries both cotangents)
            stn = next(rest for kind, _, _, rest, _ in plan_layer(exe, case, t, b, cus)[2] if kind == "stn")
            assert stn[0] > 1 and stn[1] < sp.spec_rows(s), (what, stn)
            keep = sparse_clips(b, stn[1])
        op, cots, ref_hseq, ref_grads = cached_reference(name, case, t, b, keep)
        which = 1 if sparse else 0
        run = qg.run_layer(case, op, *cots[which], device, need_dx=case["dx"])
        before = ops.spectral_layer_calls
        out = {}
        try:
            for key, value in zip(sp.KNOB_KEYS, case["knobs"]):
                if value:
                    set_knob(key, value)
            run()                                                            # (first call: allocations)
            ran = ps.kernels_run(lambda: out.update(res=run()))
            again = None if sparse else run.forward_only()
        finally:
            for key, value in zip(sp.KNOB_KEYS, case["knobs"]):
                if value:
                    set_knob(key, 0)
        assert ops.spectral_layer_calls >= before + 2, f"{what}: the layer did not take the spectral form"
        hseq, grads = out["res"]
        got = {role: {sym for sym in ran.get(role, {}) if sp.is_spectral(sym)} for role in sp.ROLES}
        print(f"spec-walk {what} ran: " + "; ".join(f"{role} = {', '.join(sorted(v))}" for role, v in got.items() if v))
        for inst, note in notes.items():
            print(f"spec-walk {what} walk: {inst}: {note}; states: {sorted(visited.get(inst, ()))}")
        for role in sp.ROLES:
            lo, hi = must.get(role, set()), must.get(role, set()) | may.get(role, set())
            assert lo <= got[role] <= hi, f"{what}: {role} ran {sorted(got[role])}, planned {sorted(lo)} (and where the recurrent kernels do not mix: {sorted(hi - lo)})"
        assert set(grads) == {"dWg", "dbg", "dWc", "dbc"} | ({"dX"} if case["dx"] else set()) | ({"dh0"} if case["h0"] else set()), sorted(grads)
        errs = {"hseq": ps.rel_err(hseq.cpu().numpy(), ref_hseq.numpy())}
        for k, g in grads.items():
            ref = ref_grads[which][k].numpy()
            errs[k] = float(abs(g.detach().cpu().double().numpy() - ref).max() / max(abs(ref).max(), 1e-6))
        print(f"spec-walk {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        all_errs[what] = errs
        if report is not None:
            report[what] = dict(errs=errs, ran=got, notes=notes, visited={i: sorted(v) for i, v in visited.items()})
        ps.assert_close(hseq.cpu().numpy(), ref_hseq.numpy(), f"{what}: hseq")
        for k, g in grads.items():
            ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[which][k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
        if sparse:
            if case["dx"]:                            # clips without a cotangent: not one bit of gradient reaches their inputs
                rest = [i for i in range(b) if i not in keep]
                assert not grads["dX"][:, rest].any(), f"{what}: dX of a clip without a cotangent is not zero"
                assert grads["dX"][:, keep].abs().amax(dim=(0, 2, 3)).min() > 0, f"{what}: a clip with a cotangent has no input gradient"
        else:
            assert torch.equal(again, hseq), f"{what}: the forward that saves nothing differs from the saving one"
    return all_errs


def product_depth(exe, cus=TABLE_CUS):
    """the deepest walk the cases of spec_plan_suite.PRODUCT_CASES reach on `cus` CUs: {kernel family: largest Q} (nnf: chunks per
    workgroup; nng: row tiles of the longest tile, 8 being a whole one; tnf: chunks per split) -- why this table exists"""
    deep = {"gemm_nnf_kernel": 0, "gemm_nng_kernel": 0, "gemm_tnf_kernel": 0}
    per_inst = {}
    for name in sp.PRODUCT_CASES:
        c = sp.CASES[name]
        for lay in range(2):
            case = dict(n=c["n"], fin=c["din"] if lay == 0 else 64, dx=lay > 0, knobs=c["knobs"])
            _, _, calls = plan_layer(exe, case, sp.T_LEN, c["b"], cus)
            s = sp.T_LEN * c["b"]
            sp_rows = sp.spec_rows(s)
            for kind, _, launches, rest, _ in calls:
                nn = launches[0] if kind == "snn" else launches[0] if kind == "sdx" and launches[0][0].startswith("gemm_nng") else None
                if nn is not None:
                    k = case["fin"] if kind == "snn" else 192
                    if nn[0].startswith("gemm_nnf_kernel"):
                        q = max(nnf_walk(k, s, sp_rows, c["n"], nn[1])[1])
                    else:
                        q = nng_walk(k, sp_rows, c["n"], nn[1])[3]
                    per_inst[nn[0]] = max(per_inst.get(nn[0], 0), q)
                elif kind == "stn" and launches[0][0].startswith("gemm_tnf_kernel"):
                    q = max(split_walk(sp_rows, rest[0], rest[1], TNF_RC))
                    per_inst[launches[0][0]] = max(per_inst.get(launches[0][0], 0), q)
    for inst, q in per_inst.items():
        deep[inst.split("<")[0]] = max(deep[inst.split("<")[0]], q)
    return deep, per_inst
