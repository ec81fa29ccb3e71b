"""The hop-diffusion kernels (csrc/kernels_diffuse.h) and the correlation-Gram kernels (csrc/kernels_graph.h) at every template instance
the launch plans of csrc/diffuse_launch.h and csrc/corr_launch.h can hand a call.  Which instance takes a call is invisible to a parity
test -- the streaming and the LDS diffusion compute the same numbers, and so do the Gram instances -- but it decides cfg2 / cfg5 time.
So this suite restates every selection rule in a few lines of Python (held against the plan driver of tests/emu over a whole grid by
tests/test_diffuse_corr_plans.py), and every case is one tiny operator call with the event recorder on: the call must launch exactly
the planned symbol under its role, and its result is compared with a float64 restatement -- the hop planes and the adjoint with
`parity_suite.assert_close` / `assert_close_scaled`, the graphs with `varlen_suite._graph_check` (sparsity pattern and 5e-6 against the
host builders, clips seeded without a top-k near-tie).  Run on the emulator and (`-m gpu`) on the MI355X by
tests/test_diffuse_corr_kernels.py.

All 43 instances are reachable without a dev knob, so the product library runs every case; the knobs (keys 5, 6, 7, 9, 18) move calls
between instances and change grids, which the goldens and the grid test pin."""
import torch

import parity_suite as ps
import varlen_suite as vs

# ---- the compiled instances, as the event recorder spells them ---------------------------------------------------------------------
FWD_STREAM, FWD_LDS = "diffuse_fwd_stream_kernel<19>", "diffuse_fwd_kernel"
ADJ_STREAM, ADJ_LDS = "diffuse_adj_stream_kernel<19>", "diffuse_adj_kernel"
FINISH = "corr_finish_kernel"


def _b(v):
    return "true" if v else "false"


def adj_rows(m):
    return f"diffuse_adj_rows_kernel<19, {m}>"


def gram(nq, rem4, ln):
    return f"corr_gram_kernel<{nq}, {_b(rem4)}, {_b(ln)}>"


def gram_rows(rem4, ln):
    return f"corr_gram_rows_kernel<{_b(rem4)}, {_b(ln)}>"


COMPILED = ({FWD_STREAM, FWD_LDS, ADJ_STREAM, ADJ_LDS, adj_rows(3), adj_rows(5), FINISH}
            | {gram(nq, r, ln) for nq in range(1, 9) for r in (False, True) for ln in (False, True)}
            | {gram_rows(r, ln) for r in (False, True) for ln in (False, True)})
KNOB_ONLY = set()                     # instances no call reaches without a dev knob


# ---- the selection rules, restated (each answers with the driver's line) -------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _rup(a, b):
    return _cdiv(a, b) * b


def _lds_stride(k):
    return k + ((2 - k % 32) + 32) % 32


LDS_BYTES, P_FLOATS, GRAM_FLOATS, ROW_CHUNK = 160 * 1024, 32 * 34, 768, 256
FINISH_LDS = (2 * 32 * 33 + 64) * 4


def diffuse_lds_bytes(n, m, fc):
    return ((m - 1) * P_FLOATS + _rup(n, 4) * _lds_stride(m * _rup(fc, 16))) * 4


def diffuse_line(adjoint, pb, s, b, n, f, m, x_bt=0, copy=0, fwd_wgs=0, adj_wgs=0, adj_lds=0, adj_planes=0):
    if not adjoint and m == 1 and not copy:
        return "none"
    sb = b if pb else 1
    streams = n == 19 and f // 4 <= 128 and s // sb >= 4
    if adjoint:                       # the knob, and 32-bit float4 offsets into Z
        streams = streams and adj_lds == 0 and s * n * m * f < 1.7e10
    if x_bt and not streams:
        return "error 2"
    if streams:
        f4, t = f // 4, s // sb
        threads = 256
        while threads > 64 and (threads // 2) // f4 >= t and threads // 2 >= f4:
            threads //= 2
        want = _cdiv((adj_wgs or 4096) if adjoint else (fwd_wgs or 1024), sb)
        ny = max(1, min(_cdiv(t, threads // f4), want))
        sym = FWD_STREAM if not adjoint else (adj_rows(m) if adj_planes == 0 and m in (3, 5) else ADJ_STREAM)
        return f"{sym} ; {sb} {ny} {threads} 0"

    def too_wide(fc):                 # the forward prefetches a sample into 4 float4 per thread
        return not adjoint and n * (fc // 4) > 1024

    fc = f
    while fc > 16 and (diffuse_lds_bytes(n, m, fc) > 96 * 1024 or too_wide(fc)):
        fc = _rup(_cdiv(fc, 2), 16)
    lds = diffuse_lds_bytes(n, m, fc)
    if lds > LDS_BYTES or too_wide(fc):
        return "error 1"
    gx, gy = (b, max(1, min(_cdiv(2048, b), s // b))) if (pb and not adjoint) else (min(s, 2048), 1)
    return f"{ADJ_LDS if adjoint else FWD_LDS} ; {gx} {gy} 256 {lds} ; x{_cdiv(f, fc)} {fc}"


def _nsplit(b, units, knob):
    return max(1, min(_cdiv(knob or 1024, b), (units + 3) // 4))


def gram_line(b, t, n, d, has_len, knob=0):
    if n < 1 or n > 32:
        return "error 1"
    if d < 4 or d % 4:
        return "error 2"
    if b < 1 or t < 1:
        return "error 3"
    ns = _nsplit(b, t, knob)
    lds = 16 * max(_rup(n * d, 256), GRAM_FLOATS)
    if lds > 64 * 1024:
        return "error 4"
    if _cdiv(d, 16) > 8:
        return "error 5"
    return f"{gram(_cdiv(d, 16), n <= 20, has_len)} ; {b} {ns} 256 {lds} ; {FINISH} ; {b} 1 256 {FINISH_LDS} ; {b * ns * GRAM_FLOATS}"


def rows_line(b, n, p, q, piece_stride, has_len, steps, knob=0):
    if n < 1 or n > 32:
        return "error 1"
    if b < 1 or p < 1:
        return "error 2"
    if q < 4 or q % 4:
        return "error 3"
    if p > 1 and (piece_stride < n * q or piece_stride % 4):
        return "error 4"
    if 4 * ((p - 1) * piece_stride * (p > 1) + n * q) >= 1 << 31:
        return "error 5"
    if has_len and p == 1 and (steps < 1 or q % steps or (q // steps) % 4):
        return "error 6"
    if has_len and p > 1 and steps != p:
        return "error 7"
    ns = min(65535, _nsplit(b, p * _cdiv(q, ROW_CHUNK), knob))
    lds = 16 * max(n * ROW_CHUNK, GRAM_FLOATS)
    return f"{gram_rows(n <= 20, has_len)} ; {b} {ns} 256 {lds} ; {FINISH} ; {b} 1 256 {FINISH_LDS} ; {b * ns * GRAM_FLOATS}"


def symbol_of(line):
    return line.split(" ; ")[0]


# ---- the cases: the smallest shapes at which each instance can still go wrong ---------------------------------------------------------
def _diffuse_cases():
    cases = {}

    def add(adjoint, pb, s, b, n, f, m, expect, launches=1):
        name = f"{'adj' if adjoint else 'fwd'}_{'clip' if pb else 'shared'}_s{s}_b{b}_n{n}_f{f}_m{m}"
        cases[name] = dict(adjoint=adjoint, pb=pb, s=s, b=b, n=n, f=f, m=m, expect=expect, launches=launches)

    # streaming: the montage, 8 samples (B = 2, T = 4); F = 100: a workgroup walks two passes; T = 5: a ragged last pass
    for adjoint, m, expect in ((False, 3, FWD_STREAM), (True, 3, adj_rows(3)), (True, 5, adj_rows(5)), (True, 2, ADJ_STREAM)):
        for pb in (0, 1):
            for s, f in ((8, 8), (8, 100), (10, 8)):
                add(adjoint, pb, s, 2, 19, f, m, expect)
    # LDS: the decoder step (fewer than 4 samples per graph), other montages, two column chunks with a ragged second one (forward:
    # the prefetch bound; the adjoint takes those rows whole)
    for adjoint, expect in ((False, FWD_LDS), (True, ADJ_LDS)):
        for pb in (0, 1):
            add(adjoint, pb, 2, 2, 19, 8, 3, expect)
        add(adjoint, 0, 8, 2, 20, 16, 3, expect)
        add(adjoint, 1, 8, 2, 5, 16, 3, expect)
        add(adjoint, 1, 4, 2, 32, 132, 3, expect, launches=1 if adjoint else 2)
    return cases


def _corr_cases():
    cases = {}
    dims = [16 * nq - 12 for nq in range(1, 9)] + [16, 128]          # the ragged quad of every NQ; whole quads at NQ = 1 and 8
    for d in dims:
        for n in (19, 21):
            for ln in (None, (6, 3)):
                cases[f"gram_d{d}_n{n}{'_len' if ln else ''}"] = dict(kind="gram", b=2, t=6, n=n, d=d, lengths=ln,
                                                                       expect=gram(_cdiv(d, 16), n <= 20, ln is not None))
    for n in (19, 21):                                                # three workgroups share a clip of 9 steps: a ragged split
        for ln in (None, (7,)):
            cases[f"gram_split_n{n}{'_len' if ln else ''}"] = dict(kind="gram", b=1, t=9, n=n, d=100, lengths=ln, expect=gram(7, n <= 20, ln is not None))
    for n in (19, 21):
        # raw rows of 520 floats: three chunks, the last one ragged; lengths: 5 steps of 104 samples
        for ln in (None, (5, 2)):
            cases[f"rows_raw_n{n}{'_len' if ln else ''}"] = dict(kind="rows", b=2, n=n, p=1, q=520, steps=5, lengths=ln, expect=gram_rows(n <= 20, ln is not None))
        # window tensors: 3 pieces of 8 floats, N * 8 apart
        for ln in (None, (3, 2)):
            cases[f"rows_win_n{n}{'_len' if ln else ''}"] = dict(kind="rows", b=2, n=n, p=3, q=8, steps=3, lengths=ln, expect=gram_rows(n <= 20, ln is not None))
    return cases


DIFFUSE_CASES = _diffuse_cases()
CORR_CASES = _corr_cases()
TOP_K = 3


def case_line(case):
    """the driver call of a case and the line the restated rules answer it with"""
    if "adjoint" in case:
        c = case
        return (f"{'dadj' if c['adjoint'] else 'dfwd'} {c['pb']} {c['s']} {c['b']} {c['n']} {c['f']} {c['m']} 0 0 0 0 0 0",
                diffuse_line(c["adjoint"], c["pb"], c["s"], c["b"], c["n"], c["f"], c["m"]))
    c, ln = case, int(case["lengths"] is not None)
    if c["kind"] == "gram":
        return f"gram {c['b']} {c['t']} {c['n']} {c['d']} {ln} 0", gram_line(c["b"], c["t"], c["n"], c["d"], ln)
    ps_ = c["n"] * c["q"] if c["p"] > 1 else 0
    return (f"grows {c['b']} {c['n']} {c['p']} {c['q']} {ps_} {ln} {c['steps'] if ln else 0} 0",
            rows_line(c["b"], c["n"], c["p"], c["q"], ps_, ln, c["steps"] if ln else 0))


# ---- one case ------------------------------------------------------------------------------------------------------------------------
def diffuse_call(name, device):
    """-> (run(): the operator call of a diffusion case on `device` -> its result, want: the float64 restatement, role)"""
    from eeg_gnn_ssl_amd import _lib, ops
    c = DIFFUSE_CASES[name]
    s, b, n, f, m, pb = c["s"], c["b"], c["n"], c["f"], c["m"], c["pb"]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    graphs = b if pb else 1
    polys = torch.randn(graphs, m - 1, n, n, generator=g) / n ** 0.5
    p64 = polys.double()[torch.arange(s) % b if pb else torch.zeros(s, dtype=torch.long)]          # (S, M-1, N, N): sample s = t * B + clip
    if not c["adjoint"]:
        x = torch.randn(s, n, f, generator=g)
        xd, pd = x.to(device), polys.to(device)
        want = torch.einsum("smij,sjf->msif", p64, x.double())
        return (lambda: ops.diffusion_hops(xd, pd, pb, b)), want, "diffuse_fwd"
    z = torch.randn(s, n, m * f, generator=g)
    zd, pd = z.to(device), polys.to(device)
    lib = _lib.get_lib()

    def run():
        dx = torch.full((s, n, f), float("nan"), device=device)
        lib.call("eeg_dcrnn_diffuse_adj", ops._p(zd), ops._p(pd), pb, s, b, n, f, m, ops._p(dx), ops._stream(zd))
        return dx
    slots = z.double().reshape(s, n, m, f)
    want = slots[:, :, 0] + torch.einsum("smji,sjmf->sif", p64, slots[:, :, 1:])
    return run, want, "diffuse_adj"


def check_diffuse_case(name, device):
    c = DIFFUSE_CASES[name]
    run, want, role = diffuse_call(name, device)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=run()))
    if not c["adjoint"]:
        ps.assert_close(out["res"].cpu().numpy(), want.numpy(), f"{name}: hop planes")
    else:
        ps.assert_close_scaled(out["res"].cpu().numpy(), want.numpy(), f"{name}: adjoint")
    assert ran == {role: {c["expect"]: c["launches"]}}, (name, ran)


def corr_call(name, device):
    """-> (call(): the operator call of a correlation case on `device` -> (adj, s1, s2), role, the host rows, valid steps per clip, width)"""
    c = CORR_CASES[name]
    b, n, lengths = c["b"], c["n"], c["lengths"]
    if c["kind"] == "gram":
        steps, width = c["t"], c["d"]
    else:
        steps, width = (c["steps"], c["q"] // c["steps"]) if c["p"] == 1 else (c["p"], c["q"])
    valid = list(lengths) if lengths else [steps] * b
    rows = vs._seeded_rows(b, n, steps, width, valid, TOP_K, first_seed=sum(map(ord, name)))          # (B, N, steps * width), no near-tie
    x = torch.from_numpy(rows)
    if c["kind"] == "gram" or c["p"] > 1:                             # (B, T, N, D); behind a clip's end every value is hostile
        x = x.reshape(b, n, steps, width).permute(0, 2, 1, 3).contiguous()
        if lengths:
            x[~vs._valid(torch.tensor(valid), steps)] = -18.4
    elif lengths:
        x = vs._hostile(x, valid, width, 1e3)
    xd = x.to(device)
    ln = torch.tensor(valid, dtype=torch.int64, device=device) if lengths else None
    op = torch.ops.eeg_dcrnn
    if c["kind"] == "gram":
        call = (lambda: op.corr_graph_len(xd, TOP_K, ln)) if lengths else (lambda: op.corr_graph(xd, TOP_K))
        role = "corr_gram_len" if lengths else "corr_gram"
    else:
        call = (lambda: op.corr_graph_rows_len(xd, TOP_K, ln, steps)) if lengths else (lambda: op.corr_graph_rows(xd, TOP_K))
        role = "corr_gram_rows_len" if lengths else "corr_gram_rows"
    return call, role, rows, valid, width


def check_corr_case(name, device):
    c = CORR_CASES[name]
    call, role, rows, valid, width = corr_call(name, device)
    out = {}
    ran = ps.kernels_run(lambda: out.update(res=call()))
    adj, s1, s2 = (t.cpu().numpy() for t in out["res"])
    for i in range(c["b"]):
        vs._graph_check(adj[i], s1[i], s2[i], rows[i][:, :valid[i] * width], TOP_K, (name, i))
    assert ran == {role: {c["expect"]: 1}, "corr_finish": {FINISH: 1}}, (name, ran)
