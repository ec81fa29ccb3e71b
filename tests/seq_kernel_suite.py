"""The recurrent kernels (csrc/kernels_seq.h: seq_fwd_kernel, seq_bwd_kernel, their two-wave forms seq_fwd2_kernel / seq_bwd2_kernel with
and without SPEC; csrc/kernels_seq_stream.h: seq_bwd_stream_kernel) at every template instance the launch plans of csrc/seq_launch.h can
hand a layer.  Which of them takes a shape is invisible to a parity test -- they compute the same recurrence -- so every case here is ONE
DCGRU layer (the operands, float64 reference and layer driver of tests/quad_gemm_suite.py) with the event recorder on: `seq_fwd` and
`seq_bwd` must each go out once, as the kernel the case names, before hidden sequence and gradients are compared.  The plan driver of
tests/emu says, without a GPU, what a layer is planned with and which instances are reachable at all; CASES must cover exactly that
set.  These kernels have no row threshold, so the shapes are the smallest that reach the instance: 2..5 clips of 1..3 steps, except
where the clip count is the point -- 383 / 384 clips (the two sides of the streamed BPTT rule) and the WALK cases with one clip more
than the grid, in which exactly one workgroup takes a second clip (per clip the kernels re-zero LDS tiles, reload the hop polynomials
and clear or load the initial state).  Run by tests/test_seq_kernels.py on the MI355X library and, for the small cases and the
instances only dev knobs reach, by tests/test_emu_parity.py on the emulator.

`python tests/seq_kernel_suite.py` evaluates the reference in fp32 on the host (the level of a correct fp32 evaluation: it
must stay below a fifth of every tolerance, else the operands are badly scaled); `--device cuda|cpu --out FILE` adds the kernels'
errors and writes the table of profiles/seq_kernel_parity.txt; `--record FILE` rewrites tests/golden/seq_plans_v1.json from the plan
driver's own output."""
import json
import os
import subprocess
import sys

if __name__ == "__main__":                # (as a script: the paths tests/conftest.py sets up)
    sys.path[1:1] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")]
import torch

import parity_suite as ps
import quad_gemm_suite as qg

HS, MS = (16, 32, 64), (1, 2, 3, 4, 5, 7)
KINDS = ("one_wave", "two_wave", "two_wave_spec", "stream")           # SeqKind of seq_launch.h, in its order
REACH = 1 << 29                                                       # floats one buffer descriptor reaches: under 2 GB
GRAD_TOL = qg.GRAD_TOL
SEQ_GRID, STREAM_GRID, LDS_BYTES = 256, 512, 160 * 1024               # one workgroup per CU / two for the streamed kernel; the LDS of a CU
# dev knobs of include/eeg_dcrnn_dev.h that the plans read: forward / backward one-wave, forward / backward no-SPEC, streamed BPTT
KNOB_FWD_ONE_WAVE, KNOB_BWD_ONE_WAVE, KNOB_FWD_NO_SPEC, KNOB_BWD_NO_SPEC, KNOB_STREAM = 12, 13, 22, 21, 3


# ---- kernel symbols as the event recorder spells them ---------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def fwd1(h, m, nks, probe=False):
    return f"seq_fwd_kernel<{h}, {m}, {nks}, {_b(probe)}>"


def bwd1(h, m, nks, probe=False):
    return f"seq_bwd_kernel<{h}, {m}, {nks}, {_b(probe)}>"


def fwd2(m, spec=False, probe=False):
    return f"seq_fwd2_kernel<64, {m}, 5, {_b(probe)}, {_b(spec)}>"


def bwd2(m, spec=False, probe=False):
    return f"seq_bwd2_kernel<64, {m}, 5, {_b(probe)}, {_b(spec)}>"


def stream(m):
    return f"seq_bwd_stream_kernel<64, {m}>"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _case(h, filt, k, n, fin, t, b, act, fwd, bwd, h0=False, lengths=False, p_batched=1, spectral=False):
    """h units, (filter, k) -> M hop matrices, n nodes, fin input features, t steps of b clips.  p_batched = 0: ONE graph for all clips in
    its 2-D form -- a non-symmetric one (general path) unless `spectral`: then the scaled Laplacian of an undirected graph, handed
    to the layer with its eigenbasis (the spectral form of the hoisted GEMMs where spec_launch.h covers the shape).  lengths: ragged
    clip lengths with clip 0 of length t and the last clip of length 1."""
    assert p_batched == 0 or not spectral
    return dict(h=h, filt=filt, k=k, n=n, fin=fin, t=t, b=b, act=act, h0=h0, lengths=lengths, len1=lengths, p_batched=p_batched, spectral=spectral,
                sup="symmetric" if spectral else ("per_clip" if p_batched else "shared"), bm=False, expect={"seq_fwd": fwd, "seq_bwd": bwd})


LAP, RW, DUAL = "laplacian", "random_walk", "dual_random_walk"        # M = k + 1, k + 1, 2k + 1
# relu only at small clip counts: its gradient jumps where a candidate pre-activation is within rounding of zero, and among the 10^5 .. 10^6
# of them in a case of 257 or more clips one such element is likely -- a correct fp32 evaluation on the host then misses the float64
# gradients by 3e-2 (measured on the 257-clip case at 32 units), which says nothing about a kernel
CASES = {
    # ---- 16 units: the one-wave kernels at every hop count, N <= 20 (NKS = 5) and above (NKS = 8) ----
    "h16_m1_n1": _case(16, RW, 0, 1, 4, 3, 2, "tanh", fwd1(16, 1, 5), bwd1(16, 1, 5), h0=True),
    "h16_m2_n15": _case(16, RW, 1, 15, 8, 3, 3, "relu", fwd1(16, 2, 5), bwd1(16, 2, 5), lengths=True, p_batched=0),
    "h16_m3_n19": _case(16, DUAL, 1, 19, 12, 2, 4, "tanh", fwd1(16, 3, 5), bwd1(16, 3, 5)),
    "h16_m4_n20": _case(16, LAP, 3, 20, 4, 1, 5, "relu", fwd1(16, 4, 5), bwd1(16, 4, 5), h0=True),
    "h16_m5_n2": _case(16, DUAL, 2, 2, 20, 3, 2, "tanh", fwd1(16, 5, 5), bwd1(16, 5, 5), lengths=True),
    "h16_m7_n17": _case(16, DUAL, 3, 17, 8, 2, 3, "tanh", fwd1(16, 7, 5), bwd1(16, 7, 5), h0=True),
    "h16_m1_n21": _case(16, LAP, 0, 21, 8, 2, 2, "relu", fwd1(16, 1, 8), bwd1(16, 1, 8)),
    "h16_m2_n21_walk": _case(16, LAP, 1, 21, 4, 2, 257, "tanh", fwd1(16, 2, 8), bwd1(16, 2, 8), h0=True),
    "h16_m3_n32": _case(16, LAP, 2, 32, 4, 3, 2, "tanh", fwd1(16, 3, 8), bwd1(16, 3, 8), lengths=True),
    "h16_m4_n31": _case(16, RW, 3, 31, 8, 1, 3, "relu", fwd1(16, 4, 8), bwd1(16, 4, 8)),
    "h16_m5_n24": _case(16, DUAL, 2, 24, 12, 2, 2, "tanh", fwd1(16, 5, 8), bwd1(16, 5, 8), h0=True),
    "h16_m7_n32": _case(16, DUAL, 3, 32, 4, 2, 2, "relu", fwd1(16, 7, 8), bwd1(16, 7, 8), lengths=True),
    # ---- 32 units ----
    "h32_m1_n16": _case(32, LAP, 0, 16, 16, 3, 3, "relu", fwd1(32, 1, 5), bwd1(32, 1, 5), lengths=True),
    "h32_m2_n20": _case(32, LAP, 1, 20, 4, 2, 2, "tanh", fwd1(32, 2, 5), bwd1(32, 2, 5), h0=True),
    "h32_m3_n1": _case(32, DUAL, 1, 1, 8, 3, 4, "tanh", fwd1(32, 3, 5), bwd1(32, 3, 5)),
    "h32_m4_n19_walk": _case(32, LAP, 3, 19, 4, 2, 257, "tanh", fwd1(32, 4, 5), bwd1(32, 4, 5), h0=True, lengths=True),
    "h32_m5_n17": _case(32, DUAL, 2, 17, 4, 1, 2, "tanh", fwd1(32, 5, 5), bwd1(32, 5, 5), h0=True),
    "h32_m7_n15": _case(32, DUAL, 3, 15, 12, 3, 2, "tanh", fwd1(32, 7, 5), bwd1(32, 7, 5)),
    "h32_m1_n32": _case(32, LAP, 0, 32, 4, 1, 4, "tanh", fwd1(32, 1, 8), bwd1(32, 1, 8), h0=True),
    "h32_m2_n31": _case(32, RW, 1, 31, 8, 3, 2, "relu", fwd1(32, 2, 8), bwd1(32, 2, 8), p_batched=0),
    "h32_m3_n21": _case(32, LAP, 2, 21, 20, 2, 3, "tanh", fwd1(32, 3, 8), bwd1(32, 3, 8), lengths=True),
    "h32_m4_n22": _case(32, LAP, 3, 22, 4, 3, 2, "tanh", fwd1(32, 4, 8), bwd1(32, 4, 8), h0=True),
    "h32_m5_n32": _case(32, DUAL, 2, 32, 8, 2, 2, "relu", fwd1(32, 5, 8), bwd1(32, 5, 8)),
    "h32_m7_n21": _case(32, DUAL, 3, 21, 4, 2, 5, "tanh", fwd1(32, 7, 8), bwd1(32, 7, 8), h0=True, lengths=True),
    # ---- 64 units above 20 nodes: one wave per SIMD at every hop count (M = 7 does not fit the LDS there and is refused) ----
    "h64_m1_n21": _case(64, LAP, 0, 21, 4, 3, 2, "tanh", fwd1(64, 1, 8), bwd1(64, 1, 8), h0=True),
    "h64_m2_n32": _case(64, LAP, 1, 32, 8, 2, 3, "relu", fwd1(64, 2, 8), bwd1(64, 2, 8), lengths=True),
    "h64_m3_n31_walk": _case(64, DUAL, 1, 31, 4, 1, 257, "tanh", fwd1(64, 3, 8), bwd1(64, 3, 8), h0=True),
    "h64_m4_n24": _case(64, LAP, 3, 24, 4, 2, 2, "tanh", fwd1(64, 4, 8), bwd1(64, 4, 8)),
    "h64_m5_n21": _case(64, DUAL, 2, 21, 12, 3, 2, "relu", fwd1(64, 5, 8), bwd1(64, 5, 8), h0=True),
    # ---- 64 units, N <= 20, M >= 4: one wave per SIMD; M = 7: the BPTT tiles with 20 node rows; from 384 clips on the streamed BPTT ----
    "h64_m4_b383": _case(64, LAP, 3, 19, 4, 1, 383, "tanh", fwd1(64, 4, 5), bwd1(64, 4, 5), h0=True),
    "h64_m4_b384": _case(64, LAP, 3, 19, 4, 1, 384, "tanh", fwd1(64, 4, 5), stream(4), h0=True),
    "h64_m5_n20": _case(64, DUAL, 2, 20, 8, 3, 3, "relu", fwd1(64, 5, 5), bwd1(64, 5, 5), lengths=True),
    "h64_m5_b513_walk": _case(64, DUAL, 2, 19, 4, 2, 513, "tanh", fwd1(64, 5, 5), stream(5), h0=True, lengths=True),
    "h64_m7_n2": _case(64, DUAL, 3, 2, 4, 3, 2, "relu", fwd1(64, 7, 5), bwd1(64, 7, 5), lengths=True),
    "h64_m7_n19_walk": _case(64, DUAL, 3, 19, 4, 2, 257, "tanh", fwd1(64, 7, 5), bwd1(64, 7, 5), h0=True),
    # ---- 64 units, N <= 20, M <= 3: two waves per SIMD ----
    "h64_m1_n16": _case(64, LAP, 0, 16, 4, 1, 2, "tanh", fwd2(1), bwd2(1)),
    "h64_m1_n17_walk": _case(64, LAP, 0, 17, 4, 2, 257, "tanh", fwd2(1), bwd2(1), h0=True),
    "h64_m2_n1": _case(64, RW, 1, 1, 8, 3, 3, "tanh", fwd2(2), bwd2(2), lengths=True, p_batched=0),
    "h64_m3_n19": _case(64, DUAL, 1, 19, 20, 3, 5, "tanh", fwd2(3), bwd2(3)),
    # a spectral layer below 16 nodes: the hoisted GEMMs run in the eigenbasis, the recurrence on the plain two-wave kernels
    "h64_m3_n15_spectral": _case(64, LAP, 2, 15, 64, 3, 4, "tanh", fwd2(3), bwd2(3), h0=True, p_batched=0, spectral=True),
    # ---- their SPEC form: a spectral layer of 16 to 20 nodes (its input gradient needs Fin = 64) ----
    "h64_m2_n16_spec": _case(64, LAP, 1, 16, 64, 3, 3, "relu", fwd2(2, spec=True), bwd2(2, spec=True), lengths=True, p_batched=0, spectral=True),
    "h64_m3_n20_spec": _case(64, LAP, 2, 20, 64, 3, 2, "tanh", fwd2(3, spec=True), bwd2(3, spec=True), h0=True, lengths=True, p_batched=0, spectral=True),
    "h64_m3_n19_spec_walk": _case(64, LAP, 2, 19, 64, 2, 257, "tanh", fwd2(3, spec=True), bwd2(3, spec=True), h0=True, p_batched=0, spectral=True),
}
# one clip more than the grid: exactly one workgroup walks on to a second clip.  Also run with the cotangent on four clips only.
WALK_CASES = tuple(name for name in CASES if name.endswith("_walk"))

# The one-wave kernels at 64 units, M <= 3, N <= 20: a product build hands them a call only where a tensor of the call is beyond the
# 2 GB a buffer descriptor reaches (the two-wave kernels go through descriptors) -- no test allocates that.  They run on the emulator
# under the one-wave dev knobs (KNOB_CASES below), with the same checks.
EXCLUDED = {sym: "reached only beyond 2 GB in a product build; runs on the emulator under dev knobs 12 / 13"
            for m in (1, 2, 3) for sym in (fwd1(64, m, 5), bwd1(64, m, 5))}

# name -> (case of the table, dev knobs, the kernels the layer then runs): instances no product build reaches below 2 GB, or at all
_ONE_WAVE = {KNOB_FWD_ONE_WAVE: 1, KNOB_BWD_ONE_WAVE: 1}
KNOB_CASES = {
    "one_wave_m1": ("h64_m1_n16", _ONE_WAVE, {"seq_fwd": fwd1(64, 1, 5), "seq_bwd": bwd1(64, 1, 5)}),
    "one_wave_m2": ("h64_m2_n1", _ONE_WAVE, {"seq_fwd": fwd1(64, 2, 5), "seq_bwd": bwd1(64, 2, 5)}),
    "one_wave_m3": ("h64_m3_n19", _ONE_WAVE, {"seq_fwd": fwd1(64, 3, 5), "seq_bwd": bwd1(64, 3, 5)}),
    "stream_m1": ("h64_m1_n16", {KNOB_STREAM: 1}, {"seq_fwd": fwd2(1), "seq_bwd": stream(1)}),
    "stream_m2": ("h64_m2_n1", {KNOB_STREAM: 1}, {"seq_fwd": fwd2(2), "seq_bwd": stream(2)}),
    "stream_m3": ("h64_m3_n19", {KNOB_STREAM: 1}, {"seq_fwd": fwd2(3), "seq_bwd": stream(3)}),
    "stream_m5": ("h64_m5_n20", {KNOB_STREAM: 1}, {"seq_fwd": fwd1(64, 5, 5), "seq_bwd": stream(5)}),      # (a product build: from 384 clips on)
}
# the emulator's share of the table: clip counts of at most 5, at least one case per kernel template and per H
EMU_CASES = ("h16_m3_n19", "h16_m7_n32", "h32_m1_n16", "h32_m5_n32", "h64_m1_n21", "h64_m5_n20", "h64_m7_n2", "h64_m3_n19", "h64_m3_n15_spectral",
             "h64_m2_n16_spec", "h64_m3_n20_spec")


def hops(case):
    return qg.hops(case)


def grid_of(case):
    return STREAM_GRID if case["expect"]["seq_bwd"].startswith("seq_bwd_stream_kernel") else SEQ_GRID


def template_of(symbol):
    """kernel template + what else selects its code path: NKS of the one-wave kernels, SPEC of the two-wave ones"""
    name, args = symbol.split("<")
    args = args.rstrip(">").split(", ")
    if name in ("seq_fwd_kernel", "seq_bwd_kernel"):
        return f"{name} NKS={args[2]}"
    return f"{name} SPEC={args[4]}" if name in ("seq_fwd2_kernel", "seq_bwd2_kernel") else name


# ---- what a layer plans: the calls of csrc/api.cpp restated, answered by the plan driver ------------------------------------------
def spec_rows(s):
    return (s + 15) // 16 * 16


def call_line(direction, h, m, n, t, b, plane_stride=0, spectral=0, sp=0, spe=0, one_wave=0, no_spec=0, stream_knob=0, probe=0):
    """one driver line: every field of SeqCall (seq_launch.h) in its order"""
    return f"s{direction} {h} {m} {n} {t} {b} {plane_stride} {spectral} {sp} {spe} {one_wave} {no_spec} {stream_knob} {probe}"


def layer_calls(h, m, n, t, b, spectral=False, knobs=None, probe=0):
    """the two driver lines of one layer, as eeg_dcrnn_layer_fwd / _bwd of api.cpp build their calls (seq_fwd_call, seq_bwd_call).
    spectral: the layer runs the spectral form.  The general-path forward leaves hop planes (T + 1 slots of B x N x H) behind, the
    spectral one U^T h instead (no plane stride); the backward states the transformed row counts whether the layer is spectral or not."""
    k = knobs or {}
    sp = spec_rows(t * b)
    fwd = call_line("fwd", h, m, n, t, b, 0, 1, sp, b + sp, k.get(KNOB_FWD_ONE_WAVE, 0), k.get(KNOB_FWD_NO_SPEC, 0), 0, probe) if spectral else \
        call_line("fwd", h, m, n, t, b, (t + 1) * b * n * h, 0, 0, 0, k.get(KNOB_FWD_ONE_WAVE, 0), k.get(KNOB_FWD_NO_SPEC, 0), 0, probe)
    bwd = call_line("bwd", h, m, n, t, b, 0, int(spectral), sp, b + sp, k.get(KNOB_BWD_ONE_WAVE, 0), k.get(KNOB_BWD_NO_SPEC, 0), k.get(KNOB_STREAM, 0), probe)
    return [fwd, bwd]


def drive(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def parse_plan(line):
    kind, probe, nks, block, grid, lds, error = (int(v) for v in line.split())
    return dict(kind=KINDS[kind], probe=bool(probe), nks=nks, block=block, grid=grid, lds=lds, error=error)


def symbol_of(direction, h, m, plan):
    """the instantiation that executes a plan (the template switch of csrc/seq_inst.cpp / seqs_inst.cpp); None: the plan is an error"""
    if plan["error"]:
        return None
    if plan["kind"] == "stream":
        return stream(m)
    if plan["kind"] == "one_wave":
        return (fwd1 if direction == "fwd" else bwd1)(h, m, plan["nks"], plan["probe"])
    assert h == 64 and plan["nks"] == 5, plan
    return (fwd2 if direction == "fwd" else bwd2)(m, spec=plan["kind"] == "two_wave_spec", probe=plan["probe"])


def planned(exe, layers):
    """layers: list of dict(h, m, n, t, b, fin, spectral (the layer is handed an eigenbasis), knobs) -> per layer {"seq_fwd": symbol,
    "seq_bwd": symbol} or None where the layer is refused (either plan reports an error: eeg_dcrnn_supported).  A layer with a basis
    takes the spectral form where spec_launch.h covers the shape with an input gradient (ops.dcgru_layer_ex), else the general path."""
    asked = [i for i, lay in enumerate(layers) if lay.get("spectral")]
    spectral = set()
    if asked:
        ok = drive(exe, [f"sup {layers[i]['t']} {layers[i]['b']} {layers[i]['n']} {layers[i]['h']} {layers[i]['fin']} {layers[i]['m']} 1" for i in asked])
        spectral = {i for i, o in zip(asked, ok) if o == "1"}
    lines = [ln for i, lay in enumerate(layers) for ln in layer_calls(lay["h"], lay["m"], lay["n"], lay["t"], lay["b"], i in spectral, lay.get("knobs"))]
    out = drive(exe, lines)
    res = []
    for i, lay in enumerate(layers):
        f, b = parse_plan(out[2 * i]), parse_plan(out[2 * i + 1])
        res.append(None if f["error"] or b["error"] else {"seq_fwd": symbol_of("fwd", lay["h"], lay["m"], f), "seq_bwd": symbol_of("bwd", lay["h"], lay["m"], b)})
    return res


def case_layer(case, knobs=None):
    return dict(h=case["h"], m=hops(case), n=case["n"], t=case["t"], b=case["b"], fin=case["fin"], spectral=case["spectral"], knobs=knobs)


ENUM_CLIPS = (1, 255, 256, 257, 383, 384, 511, 512, 513)


def reachable_instances(exe):
    """every kernel symbol some supported layer is planned with, no dev knobs: 16 / 32 / 64 units x every supported hop count x 1 .. 32
    nodes x clip counts on both sides of 256 / 384 / 512 x with and without an eigenbasis (Fin = 64, as its input gradient needs), and
    per (units, hops, nodes) one layer of 256 clips whose hidden sequence is past the 2 GB a descriptor reaches -> (below, beyond)"""
    shapes = [(h, m, n) for h in HS for m in MS for n in range(1, 33)]
    below = [dict(h=h, m=m, n=n, t=2, b=b, fin=64, spectral=s) for h, m, n in shapes for b in ENUM_CLIPS for s in (False, True)]
    beyond = [dict(h=h, m=m, n=n, t=REACH // (256 * n * h) + 1, b=256, fin=64, spectral=s) for h, m, n in shapes for s in (False, True)]
    assert all(lay["t"] * lay["b"] * lay["n"] * lay["h"] >= REACH for lay in beyond)
    sets = []
    for layers in (below, beyond):
        sets.append({s for roles in planned(exe, layers) if roles is not None for s in roles.values()})
    return sets[0], sets[1]


# ---- the recorded selection (tests/golden/seq_plans_v1.json) --------------------------------------------------------------------
def recorded_calls():
    """(calls for the development build of the driver, calls for the product build): both sides of every rule edge of seq_launch.h"""
    dev = []
    # as a layer states its calls, one axis at a time (a cross product of the axes would pin nothing more and fill the file):
    # every supported (H, M) at the last node count of NKS = 5 and the first of NKS = 8 (the LDS of each instance; 64 units x M = 7 above
    # 20 nodes does not fit), and unsupported widths and hop counts
    for h, m in [(h, m) for h in HS for m in MS] + [(8, 3), (48, 3), (64, 0), (64, 6), (64, 8)]:
        for n in (20, 21):
            dev += layer_calls(h, m, n, 2, 4)
    # the node counts at the edges of NKS and of the SPEC form, spectral or not, without a hop (no SPEC form) and with two
    for m in (1, 3):
        for n in (1, 15, 16, 20, 21, 32):
            for s in (False, True):
                dev += layer_calls(64, m, n, 2, 4, s)
    # the clip counts at the edges of the two grids and of the streamed rule: where the two-wave kernels run (M = 3) and where the
    # streamed one may (M = 5); the rule's other conditions: M = 4 on both sides, more than 20 nodes, 32 units
    for m in (3, 5):
        for b in ENUM_CLIPS:
            dev += layer_calls(64, m, 19, 2, b)
    for h, m, n, b in ((64, 4, 19, 383), (64, 4, 19, 384), (64, 5, 21, 384), (32, 5, 19, 384), (64, 3, 19, 384)):
        dev += layer_calls(h, m, n, 2, b, h == 64 and m == 3)
    # the 2 GB reach, one step below and at it, each product on its own (64 units, 16 nodes: N*H = 1024, N*3H = 3072) under a spectral
    # call (every rule reads its size); the sizes the general path reads once more without; the plane stride at other hop counts
    t_h, t_3h = REACH // 1024, REACH // 3072
    for d in ("fwd", "bwd"):
        for s in (1, 0):
            sp = (s, 64, 80)
            dev += [call_line(d, 64, 3, 16, t, 1, 0, *sp) for t in (t_h - 1, t_h)]                                     # T*B*N*H
            dev += [call_line(d, 64, 3, 16, t, 1, 0, *sp) for t in (t_3h, t_3h + 1)]                                   # T*B*N*3H (3072 does not divide 2^29)
            dev += [call_line(d, 64, 3, 16, 2, 4, v, *sp) for v in ((REACH - 1) // 2, REACH // 2)]                     # (M-1)*plane_stride
        dev += [call_line(d, 64, 3, 16, 2, 4, 0, 1, v, 80) for v in (t_3h, t_3h + 1)]                                  # N*Sp*3H
        dev += [call_line(d, 64, 3, 16, 2, 4, 0, 1, 64, v) for v in (t_h - 1, t_h)]                                    # N*SpE*H
    dev += [call_line("fwd", 64, m, 16, 2, 4, v) for m in (1, 2) for v in (REACH - 1, REACH)]                          # (M = 1: no planes, no limit)
    dev += [call_line("bwd", 64, 5, 16, t, 512) for t in (341, 342)]                                                   # the streamed kernel's dXW: 512*3072*T
    # each knob alone, and the probe flag (with and without the one-wave knobs): a SPEC shape, a two-wave one, streamed and not
    shapes = [(64, 3, 19, 4, True), (64, 3, 19, 4, False), (64, 5, 19, 4, False), (64, 5, 19, 384, False), (64, 3, 21, 4, False)]
    knobbed = []
    for h, m, n, b, s in shapes:
        for knobs in ({KNOB_FWD_ONE_WAVE: 1}, {KNOB_BWD_ONE_WAVE: 1}, {KNOB_FWD_NO_SPEC: 1}, {KNOB_BWD_NO_SPEC: 1}, {KNOB_STREAM: 1}, {KNOB_STREAM: 2}):
            dev += layer_calls(h, m, n, 2, b, s, knobs)
        knobbed += layer_calls(h, m, n, 2, b, s, None, probe=1) + layer_calls(h, m, n, 2, b, s, _ONE_WAVE, probe=1)
    dev += knobbed
    # the product build: the probe flag (no probe instantiation exists there) and the same shapes without it; the table's own layers are
    # planned with that build by tests/test_seq_kernels.py
    product = list(knobbed)
    for h, m, n, b, s in shapes:
        product += layer_calls(h, m, n, 2, b, s)
    return dev, product


def record(exe_dev, exe_product, path):
    dev, product = recorded_calls()
    doc = {"about": "launch plans of csrc/seq_launch.h as the plan driver printed them (tests/emu/gemm_plan_driver.cpp: sfwd / sbwd lines): "
                    "kind probe nks block grid lds error.  plans: driver built with -DEEG_DEV; plans_product: without",
           "plans": [{"call": c, "plan": p} for c, p in zip(dev, drive(exe_dev, dev))],
           "plans_product": [{"call": c, "plan": p} for c, p in zip(product, drive(exe_product, product))]}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: ' + (json.dumps(v) if isinstance(v, str) else "[\n  " + ",\n  ".join(json.dumps(e) for e in v) + "\n ]")
                                   for k, v in doc.items()) + "\n}\n")
    return doc


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------
def sparse_clips(b, grid):
    """first clip, the last clip of the grid's first round, the one clip of its second round (= the last clip: b = grid + 1)"""
    return sorted({0, grid - 1, grid, b - 1})


_REF_CACHE = {}


def cached_reference(name, seed=0):
    """(operands, cotangents, reference hseq, reference gradients per cotangent) of a case, computed once per process: the dense
    cotangent and -- WALK_CASES -- the one that lives on sparse_clips only"""
    key = (name, seed)
    if key not in _REF_CACHE:
        case = CASES[name]
        op = qg.make_operands(case, case["t"], case["b"], seed)
        cots = [(op["w"], op["wsel"])]
        if name in WALK_CASES:
            keep = torch.zeros(case["b"], dtype=torch.bool)
            keep[sparse_clips(case["b"], grid_of(case))] = True
            cots.append((op["w"] * keep.view(1, -1, 1), op["wsel"] * keep.view(-1, 1)))
        hseq, grads = qg.reference(case, op, cots)
        _REF_CACHE[key] = (op, cots, hseq, grads)
    return _REF_CACHE[key]


def errors(hseq, grads, ref_hseq, ref_grads):
    errs = {"hseq": ps.rel_err(hseq.cpu().numpy(), ref_hseq.numpy())}
    for k, g in grads.items():
        ref = ref_grads[k].numpy()
        errs[k] = float(abs(g.detach().cpu().double().numpy() - ref).max() / max(abs(ref).max(), 1e-6))
    return errs


def yardstick(name, seed=0):
    """the reference's own arithmetic in fp32 on the host against the float64 reference: {tensor: error} for the dense cotangent"""
    case = CASES[name]
    op, cots, ref_hseq, ref_grads = cached_reference(name, seed)
    hseq, grads = qg.reference(case, op, cots[:1], dtype=torch.float32)
    grads = {k: g for k, g in grads[0].items() if k != "dh0" or case["h0"]}
    return errors(hseq, grads, ref_hseq, ref_grads[0])


# ---- the layer under test -------------------------------------------------------------------------------------------------------
def assert_ran(ran, expect, what):
    """the recorder's {role: {symbol: launches}} of ONE forward + backward: seq_fwd and seq_bwd went out once each, as the expected kernel"""
    got = {role: ran.get(role, {}) for role in ("seq_fwd", "seq_bwd")}
    want = {role: {sym: 1} for role, sym in expect.items()}
    assert got == want, f"{what}: recurrent kernels that ran {got}, expected {want}"


def check_case(name, device, sparse=False, seed=0, report=None, expect=None):
    """One case: the layer on `device` against the float64 reference (hseq under assert_close, every gradient under
    assert_close_scaled(tol=5e-5)), after the proof that the expected kernels took the recurrence; then the forward once more under
    torch.no_grad() (the kernel saves nothing for a backward: Rs == nullptr), bit for bit the same hidden sequence.  sparse (WALK_CASES):
    the cotangent lives on sparse_clips only, so that a clip dropped, doubled or misplaced in the walk is measured against four clips'
    worth of gradient, and no other clip's input may receive one bit of it.  expect: the kernels under dev knobs (KNOB_CASES)."""
    case = CASES[name]
    assert not sparse or name in WALK_CASES
    op, cots, ref_hseq, ref_grads = cached_reference(name, seed)
    which = 1 if sparse else 0
    run = qg.run_layer(case, op, *cots[which], device)
    run()                                                                                 # (first call: allocations)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=run()))
    hseq, grads = out["res"]
    what = f"{name}{' (sparse)' if sparse else ''} T={case['t']} B={case['b']} N={case['n']}"
    assert_ran(ran, expect if expect is not None else case["expect"], what)
    if case["spectral"]:                          # the layer did take the spectral form: U Yh as a pass of its own exactly where the kernel does not mix
        assert "gemm_nn_xw" in ran and ("spec_mix_y" in ran) == (not case["expect"]["seq_fwd"].endswith("true>")), f"{what}: {sorted(ran)}"
    errs = errors(hseq, grads, ref_hseq, ref_grads[which])
    print(f"seq-kernel {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"seq-kernel {what} ran: " + "; ".join(f"{role} = {sym}" for role in ("seq_fwd", "seq_bwd") for sym in ran.get(role, {})))
    if report is not None:
        report[what] = errs
    ps.assert_close(hseq.cpu().numpy(), ref_hseq.numpy(), f"{what}: hseq")
    for k, g in grads.items():
        ps.assert_close_scaled(g.detach().cpu().numpy(), ref_grads[which][k].numpy(), f"{what}: {k}", tol=GRAD_TOL)
    if sparse:                                    # clips without a cotangent: not one bit of gradient reaches their inputs
        keep = sparse_clips(case["b"], grid_of(case))
        rest = [i for i in range(case["b"]) if i not in keep]
        assert not grads["dX"][:, rest].any(), f"{what}: dX of a clip without a cotangent is not zero"
        assert grads["dX"][:, keep].abs().amax(dim=(0, 2, 3)).min() > 0, f"{what}: a clip with a cotangent has no input gradient"
    else:
        again = run.forward_only()
        assert torch.equal(again, hseq), f"{what}: the forward that saves nothing differs from the saving one"
    return errs, ran


# ---- yardstick, parity table, recording -----------------------------------------------------------------------------------------
TENSORS = ("hseq", "dX", "dh0", "dWg", "dbg", "dWc", "dbc")


def _row(label, errs):
    return f"{label:<40}" + "".join(f"{errs[k]:>10.2e}" if k in errs else f"{'-':>10}" for k in TENSORS)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[-1])
    ap.add_argument("--device", choices=("cuda", "cpu"))
    ap.add_argument("--out")
    ap.add_argument("--record")
    ap.add_argument("--cases", nargs="*")
    a = ap.parse_args(argv)
    if a.record:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "p"))
            doc = record(qg.build_plan_driver(tmp), qg.build_plan_driver(os.path.join(tmp, "p"), dev=False), a.record)
        print(f"{a.record}: {len(doc['plans'])} + {len(doc['plans_product'])} plans")
        return 0
    torch.set_num_threads(16)
    names = a.cases or ([n for n in CASES if n in EMU_CASES] if a.device == "cpu" else list(CASES))
    if a.device == "cpu":
        import emu_support
        emu_support.install_emulator()
    lines = ["case" + " " * 36 + "".join(f"{k:>10}" for k in TENSORS)]
    worst = 0.0
    for name in names:
        yard = yardstick(name)
        worst = max(worst, yard["hseq"] / ps.TOL, max(v for k, v in yard.items() if k != "hseq") / GRAD_TOL)
        lines.append(_row(f"{name}  fp32 host", yard))
        if a.device:
            rep = {}
            check_case(name, a.device, report=rep)
            lines.append(_row(f"{'':<{len(name)}}  {'MI355X' if a.device == 'cuda' else 'emulator'}", next(iter(rep.values()))))
            if name in WALK_CASES and a.device == "cuda":
                check_case(name, a.device, sparse=True, report=rep)
                lines.append(_row(f"{'':<{len(name)}}  MI355X sparse", list(rep.values())[-1]))
        print(lines[-1] if not a.device else "\n".join(lines[-2:]), flush=True)
    lines.append(f"worst fp32 yardstick / tolerance: {worst:.3f} (must stay below 0.2)")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if worst < 0.2 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
