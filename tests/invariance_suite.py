"""Results depend on inputs only.  The instance tables (tests/seq_kernel_suite.py, quad_gemm_suite.py, dec_kernel_suite.py, spec_plan_suite.py,
diffuse_corr_suite.py) compare every kernel instance with a float64 reference -- after a first call that warms the allocator, so a
kernel that reads a pad row, a workspace region or a saved plane nobody wrote finds last call's correct values there and passes.
This suite takes the same cases, the same `run` closures, and asks four questions that need no reference and no tolerance: every
comparison is bit for bit, on every public result (outputs and every gradient), between runs of the same code.

  a. repeat     8 runs of forward + backward, all identical to the first (a difference is reported as nondeterminism, and b - d of that
                case are skipped: they would say nothing)
  b. poison     every allocation of the operator layer goes through `ops._new`; with that hook filling what it hands out -- floating-point
                tensors only: a poisoned index could turn a stray read into a wild access -- the results must not move.  Two fills: quiet NaN,
                and 7.0e3 (fmaxf, fminf and compare-selects swallow a NaN: relu and max paths would hide it).  Outputs come from `_new`
                too, so this also proves that every output element is written.
  c. neighbour  the case, then a "dirtier" case of the same table with operands scaled by 1e3 (the instance with the largest dynamic LDS),
                then the case again: what another kernel left in LDS and caches must not show.
  d. isolation  clips 0, middle and last keep their inputs and their batch positions, every other clip gets inputs of another seed
                scaled by 30 (x, h0, per-clip supports; lengths stay): the kept clips' outputs, input gradients and dh0 must not move (weight
                gradients sum over clips and are not compared).  Cases of two or three clips keep clip 0 (and the last of three), so that
                one clip does change.

a and c say nothing on the emulator (one lane at a time, no LDS contents); b and d run there on the tables' emulator share, and the
case's own `check_case` runs once inside the NaN context (the planned kernels still run, the float64 tolerance still holds).  The
operator-level checks (a, b) and the `TrainStep` check (clean against poisoned from construction on) follow the same pattern.
Run by tests/test_invariance.py; `python tests/invariance_suite.py --device cuda --out FILE` writes profiles/invariance_suite.txt."""
import contextlib
import os
import sys
import time

if __name__ == "__main__":                # (as a script: the paths tests/conftest.py sets up)
    sys.path[1:1] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")]
import numpy as np
import torch

import cases
import dec_kernel_suite as dk
import diffuse_corr_suite as dc
import parity_suite as ps
import quad_gemm_suite as qg
import seq_kernel_suite as sk
import spec_plan_suite as sp
from oracle import dcrnn_oracle as orc

FILLS = {"nan": float("nan"), "7e3": 7.0e3}
REPEATS = 8
DIRTY_SCALE, OTHER_SCALE = 1e3, 30.0
TABLES = ("seq", "quad", "dec", "spec", "diffuse", "corr")
# the dirtier of a table: its instance with the largest dynamic LDS.  seq_fwd_kernel / seq_bwd_kernel<64, 7, 5> (the recurrent kernels
# of the quad table's layers too); the decoder's widest CX0 (20) at its LDS edge; the spectral form's widest input
DIRTIER = {"seq": "h64_m7_n2", "quad": "h64_m7_n2", "dec": "m5_d208_l2", "spec": "n19_din200"}


# ---- bit comparison ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    """bit for bit (a NaN equals the same NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def assert_same(got, want, what):
    """two results {name: tensor} of the same call: every tensor bit-identical, the message names the ones that are not"""
    assert set(got) == set(want), f"{what}: results {sorted(got)} / {sorted(want)}"
    bad = []
    for k in want:
        if not same(got[k], want[k]):
            d = _bits(got[k]) != _bits(want[k]) if got[k].shape == want[k].shape else None
            where = "" if d is None else f" ({int(d.sum())} of {d.numel()} elements, first at flat index {int(d.reshape(-1).nonzero()[0])})"
            bad.append(f"{k}{where}")
    assert not bad, f"{what}: differ in " + ", ".join(bad)


# ---- the poison hook -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def poison(fill, patch=None):
    """`ops._new` hands out floating-point tensors filled with `fill` (integer tensors as allocated) -> {"calls", "floats"} of what it
    filled.  patch: a pytest monkeypatch (`patch.setattr(ops, "_new", ...)`); None: set and restored here (the script)."""
    from eeg_gnn_ssl_amd import ops
    clean, stats = ops._new, {"calls": 0, "floats": 0}

    def filled(shape, like, dtype=torch.float32):
        t = clean(shape, like, dtype)
        if t.is_floating_point() and t.numel():
            t.fill_(fill)
            stats["calls"] += 1
            stats["floats"] += t.numel()
        return t
    if patch is not None:
        with patch.context() as m:
            m.setattr(ops, "_new", filled)
            yield stats
    else:
        ops._new = filled
        try:
            yield stats
        finally:
            ops._new = clean


# ---- the four checks on a closure run() -> {name: tensor} ------------------------------------------------------------------------------
class Nondeterminism(AssertionError):
    pass


def check_repeat(run, what, repeats=REPEATS):
    first = run()
    for i in range(1, repeats):
        try:
            assert_same(run(), first, f"{what}: run {i + 1} of {repeats} against the first")
        except AssertionError as e:
            raise Nondeterminism(f"NONDETERMINISM {e}") from None
    return first


def check_poison(run, what, patch=None, clean=None, need_calls=True):
    """clean against each fill -> the hook's statistics of the NaN run"""
    clean = run() if clean is None else clean
    stats = None
    for label, fill in FILLS.items():
        with poison(fill, patch) as st:
            got = run()
        assert_same(got, clean, f"{what}: allocations filled with {label} against clean")
        stats = stats or dict(st)
        assert not need_calls or (st["calls"] > 0 and st["floats"] > 0), f"{what}: the poisoned ops._new was never asked for a float tensor"
    return stats


def check_neighbour(run, dirty, what, clean=None):
    clean = run() if clean is None else clean
    dirty()
    assert_same(run(), clean, f"{what}: after the dirtier case against before")


def kept_clips(b):
    return sorted({0, b // 2, b - 1}) if b > 3 else [0, 2] if b == 3 else [0]


def _mix(a, other, keep, dim, tamper=None):
    """a on the kept clips (index along dim), OTHER_SCALE * other elsewhere; tamper: a kept clip that is changed as well (the bite test)"""
    mask = torch.zeros(a.shape[dim], dtype=torch.bool)
    mask[keep] = True
    if tamper is not None:
        mask[tamper] = False
    shape = [1] * a.dim()
    shape[dim] = -1
    return torch.where(mask.view(shape), a, (OTHER_SCALE * other).to(a.dtype))


# ---- the tables: name -> run closures ----------------------------------------------------------------------------------------------------
class Env:
    """where the cases run: device, the adjacency fixture, how to set a dev knob (development builds and the emulator), the plan driver"""

    def __init__(self, device, adj3d=None, set_knob=None, exe=None):
        self.device, self.adj3d, self.set_knob, self.exe = device, adj3d, set_knob, exe
        self.emu = device == "cpu"
        self.cus = qg.EMU_CUS if self.emu else torch.cuda.get_device_properties(0).multi_processor_count

    @contextlib.contextmanager
    def knobs(self, knobs):
        knobs = {k: v for k, v in knobs.items() if v}
        assert not knobs or self.set_knob is not None, "dev knobs need a development build"
        try:
            for k, v in knobs.items():
                self.set_knob(k, v)
            yield
        finally:
            for k in knobs:
                self.set_knob(k, 0)


def table_cases(table, emu):
    """the invariance parametrisation of a table: on the MI355X every case of it, on the emulator its emulator share"""
    if table == "seq":
        return list(sk.EMU_CASES) + list(sk.KNOB_CASES) if emu else list(sk.CASES)
    if table == "quad":
        return list(qg.CASES)                                     # (tests/test_emu_parity.py runs all of them at emulator row counts)
    if table == "dec":
        return list(dk.EMU_CASES) if emu else list(dk.ALL_CASES)
    if table == "spec":
        return list(sp.CASES) if emu else list(sp.PRODUCT_CASES)  # (the knob case: development builds and the emulator)
    return list(dc.DIFFUSE_CASES if table == "diffuse" else dc.CORR_CASES)


def _seq_case(name):
    base, knobs, expect = sk.KNOB_CASES[name] if name in sk.KNOB_CASES else (name, {}, None)
    return base, sk.CASES[base], knobs, expect


def _layer_dims(table, name, env):
    if table == "seq":
        case = _seq_case(name)[1]
        return case, case["t"], case["b"]
    case = qg.CASES[name]
    t, b, _ = qg.emu_dims(case) if env.emu else qg.case_dims(case, 256 * env.cus)
    return case, t, b


def _layer_knobs(table, name, env):
    return _seq_case(name)[2] if table == "seq" else ({2: qg.EMU_KNOB_QUAD} if env.emu else {})


def _layer_run(case, op, env, knobs):
    run = qg.run_layer(case, op, op["w"], op["wsel"], env.device)

    def go():
        with env.knobs(knobs):
            hseq, grads = run()
        res = {"hseq": hseq, **grads}
        if run.hsel is not None:
            res["hsel"] = run.hsel
        return res
    return go


def _dec_run(case, op, env):
    run = dk.run_decoder(case, op, op["wout"], env.device)

    def go():
        out, grads = run()
        return {"out": out, **grads}
    return go


def _spec_run(name, env, x_scale=1.0):
    run = sp.run_model(name, env.device, env.adj3d, x_scale)

    def go():
        with env.knobs(dict(zip(sp.KNOB_KEYS, sp.CASES[name]["knobs"]))):
            logits, grads = run()
        return {"logits": logits, **grads}
    return go


def runner(table, name, env):
    """run() -> {name: tensor}: one forward + backward of the case (the tables' own closures), every public result"""
    if table in ("seq", "quad"):
        case, t, b = _layer_dims(table, name, env)
        return _layer_run(case, qg.make_operands(case, t, b, 0), env, _layer_knobs(table, name, env))
    if table == "dec":
        case = dk.ALL_CASES[name]
        return _dec_run(case, dk.make_operands(case, 0), env)
    if table == "spec":
        return _spec_run(name, env)
    if table == "diffuse":
        run = dc.diffuse_call(name, env.device)[0]
        return lambda: {"result": run()}
    call = dc.corr_call(name, env.device)[0]
    return lambda: dict(zip(("adj", "s1", "s2"), call()))


def dirtier(table, env):
    """the table's dirtier case with every floating-point operand scaled by DIRTY_SCALE"""
    name = DIRTIER[table]
    if table in ("seq", "quad"):
        case = sk.CASES[name]
        op = qg.make_operands(case, case["t"], case["b"], 3)
        op = {k: (v * DIRTY_SCALE if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in op.items()}
        return _layer_run(case, op, env, {})
    if table == "dec":
        case = dk.ALL_CASES[name]
        op = dk.make_operands(case, 3)
        op = dict(op, targets=op["targets"] * DIRTY_SCALE, h0=op["h0"] * DIRTY_SCALE, wout=op["wout"] * DIRTY_SCALE)
        return _dec_run(case, op, env)
    return _spec_run(name, env, DIRTY_SCALE)


def isolation_cases(table, emu):
    """check d: the walk cases and one more case per kernel template (the one with the most clips)"""
    if table == "seq":
        names = table_cases("seq", emu)
        best = {}
        for name in names:
            if not name.endswith("_walk"):
                base, case, _, expect = _seq_case(name)
                for sym in (expect or case["expect"]).values():
                    key = sk.template_of(sym)
                    if key not in best or case["b"] > _seq_case(best[key])[1]["b"]:
                        best[key] = name
        return [n for n in names if n.endswith("_walk") or n in best.values()]
    if table == "dec":
        names = table_cases("dec", emu)
        best = {}
        for name in names:
            case = dk.ALL_CASES[name]
            if name not in dk.WALK_CASES:
                key = (case["expect"] or {"dec_bwd_persist": "per step, "})["dec_bwd_persist"].split(", ")[-1]      # CX0 of the backward; the per-step path
                if key not in best or case["b"] > dk.ALL_CASES[best[key]]["b"]:
                    best[key] = name
        return [n for n in names if n in dk.WALK_CASES or n in best.values()]
    return []


def check_isolation(table, name, env, tamper=False):
    """check d.  tamper: the middle kept clip's x is changed as well -- the check must then fail (tests/test_invariance.py)"""
    if table in ("seq", "quad"):
        case, t, b = _layer_dims(table, name, env)
        keep = kept_clips(b)
        bad = keep[len(keep) // 2] if tamper else None
        op, other = qg.make_operands(case, t, b, 0), qg.make_operands(case, t, b, 1)
        mixed = dict(op, xb=_mix(op["xb"], other["xb"], keep, 0, bad))
        if op["h0"] is not None:
            mixed["h0"] = _mix(op["h0"], other["h0"], keep, 0)
        if case.get("sup", "per_clip") == "per_clip":
            mixed["sup"] = [_mix(s, o, keep, 0) for s, o in zip(op["sup"], other["sup"])]
        knobs = _layer_knobs(table, name, env)
        ra, rb = _layer_run(case, op, env, knobs)(), _layer_run(case, mixed, env, knobs)()
        cut = {"hseq": lambda v: v[:, keep], "dX": lambda v: v[:, keep], "hsel": lambda v: v[keep], "dh0": lambda v: v[keep]}
    else:
        assert table == "dec"
        case = dk.ALL_CASES[name]
        keep = kept_clips(case["b"])
        bad = keep[len(keep) // 2] if tamper else None
        op, other = dk.make_operands(case, 0), dk.make_operands(case, 1)
        mixed = dict(op, targets=_mix(op["targets"], other["targets"], keep, 1), h0=_mix(op["h0"], other["h0"], keep, 1, bad))
        if case["sup"] == "per_clip":
            mixed["sup"] = [_mix(s, o, keep, 0) for s, o in zip(op["sup"], other["sup"])]
        ra, rb = _dec_run(case, op, env)(), _dec_run(case, mixed, env)()
        cut = {"out": lambda v: v[:, keep], "dh0": lambda v: v[:, keep]}
    assert all(k in ra for k in cut if k not in ("hsel", "dh0")), sorted(ra)
    assert_same({k: f(rb[k]) for k, f in cut.items() if k in rb}, {k: f(ra[k]) for k, f in cut.items() if k in ra},
                f"{table} {name}: clips {keep} with the other clips' inputs replaced against the original run")
    return keep


def check_in_nan_context(table, name, env, patch=None):
    """the case's own check (the planned kernels run, the float64 tolerance holds) with every allocation NaN-filled"""
    with poison(FILLS["nan"], patch):
        if table == "seq":
            base, _, knobs, expect = _seq_case(name)
            with env.knobs(knobs):
                sk.check_case(base, env.device, expect=expect)
        elif table == "quad":
            with env.knobs(_layer_knobs(table, name, env)):
                qg.check_case(name, env.device, 256 * env.cus, exact=not env.emu, dims=qg.emu_dims(qg.CASES[name]) if env.emu else None)
        elif table == "dec":
            dk.check_case(name, env.device)
        elif table == "spec":
            sp.check_case(name, env.device, env.adj3d, env.exe, env.cus, set_knob=env.set_knob)
        elif table == "diffuse":
            dc.check_diffuse_case(name, env.device)
        else:
            dc.check_corr_case(name, env.device)


def check_table_case(table, name, env, patch=None, record=None):
    """every check the table's case gets where it runs.  MI355X: a, b, c (diffuse / corr: a, b), d where isolation_cases says;
    emulator: b, d and the case's own check inside the NaN context."""
    t0, ran, stats = time.perf_counter(), [], {"calls": 0, "floats": 0}
    what = f"{table} {name}"
    row = dict(case=what, checks=ran, stats=stats, seconds=0.0, verdict="pass")
    if record is not None:
        record.append(row)
    try:
        run = runner(table, name, env)
        if env.emu:
            clean = run()
        else:
            ran.append("a")
            clean = check_repeat(run, what)
        ran.append("b")
        # the adjoint diffusion cases call the library entry with an output of their own: nothing of theirs comes from ops._new
        needs = not (table == "diffuse" and dc.DIFFUSE_CASES[name]["adjoint"])
        stats.update(check_poison(run, what, patch, clean, need_calls=needs))
        if not env.emu and table in DIRTIER:
            ran.append("c")
            check_neighbour(run, dirtier(table, env), what, clean)
        if name in isolation_cases(table, env.emu):
            ran.append("d")
            check_isolation(table, name, env)
        if env.emu:
            ran.append("own check under NaN")
            check_in_nan_context(table, name, env, patch)
    except Nondeterminism:
        row["verdict"] = "NONDETERMINISTIC (b - d skipped)"
        raise
    except AssertionError:
        row["verdict"] = f"FAIL in {ran[-1] if ran else 'setup'}"
        raise
    finally:
        row["seconds"] = time.perf_counter() - t0
    return row


# ---- the zero-call bite: a layer above the first, whose dX has a slot only eeg_dcrnn_zero writes ----------------------------------------
def second_layer_runner(device):
    """run() -> {hseq, dX, ...} of the SECOND of two DCGRU layers, called as the encoder calls it (x = the hext of the layer below, x_off =
    1, its hop planes handed over): slot 0 of dX is written by nothing but the eeg_dcrnn_zero call of ops._dcgru_layer_bwd_impl"""
    from eeg_gnn_ssl_amd import ops
    case = dict(h=16, filt="dual_random_walk", k=1, n=19, fin=8, act="tanh", h0=True, lengths=False, sup="per_clip", bm=False)
    t, b, n, h, m = 3, 2, 19, 16, 3
    op0 = qg.make_operands(case, t, b, 0)
    op1 = qg.make_operands(dict(case, fin=h), t, b, 1)
    sup = [s.to(device) for s in op0["sup"]]
    p, pb = ops.hop_polys(sup, case["k"], b)
    par0, par1 = ({q: o[q].to(device) for q in ("wg", "bg", "wc", "bc")} for o in (op0, op1))
    x0, h0, w = op0["xb"].transpose(0, 1).contiguous().to(device), op0["h0"].to(device), op0["w"].to(device)

    def run():
        lay0 = ops.dcgru_layer_ex(x0.detach().requires_grad_(True), 0, h0, p, pb, par0["wg"], par0["bg"], par0["wc"], par0["bc"], n, h, m, "tanh")
        x1 = lay0.hext.detach().view(t + 1, b, n, h).requires_grad_(True)
        q = {k: v.detach().requires_grad_(True) for k, v in par1.items()}
        lay1 = ops.dcgru_layer_ex(x1, 1, None, p, pb, q["wg"], q["bg"], q["wc"], q["bc"], n, h, m, "tanh", x_planes=lay0.hpl.detach())
        (lay1.hseq * w).sum().backward()
        return {"hseq": lay1.hseq.detach(), "dX": x1.grad, "dWg": q["wg"].grad, "dbg": q["bg"].grad, "dWc": q["wc"].grad, "dbc": q["bc"].grad}
    return run


@contextlib.contextmanager
def without_entry(lib, entry):
    """the library object with one entry point filtered out of `call` (test side: the bite)"""
    real = lib.call
    lib.call = lambda name, *args: None if name == entry else real(name, *args)
    try:
        yield
    finally:
        del lib.call


# ---- operator level: a and b at the smallest shapes of parity_suite ---------------------------------------------------------------------
def _dconv_run(tag, env):
    from eeg_gnn_ssl_amd import DiffusionGraphConv
    from closed_form import cf
    c, dev = cases.dconv_inputs(tag, env.adj3d), env.device
    mod = DiffusionGraphConv(2 if c["filt"] == "dual_random_walk" else 1, c["din"], c["h"], 19, 2, c["o"], filter_type=c["filt"])
    ps.load(mod, {"weight": c["weight"], "biases": c["biases"]}, dev)
    sup, up = [t.to(dev) for t in c["sup"]], cases.T(cf((c["b"], 19 * c["o"]), scale=1.0, freq=0.291, phase=0.4)).to(dev)

    def run():
        mod.zero_grad(set_to_none=True)
        x, s = c["x"].to(dev).requires_grad_(True), c["s"].to(dev).requires_grad_(True)
        out = mod(sup, x, s, c["o"])
        (out * up).sum().backward()
        return {"out": out.detach(), "dx": x.grad, "ds": s.grad, "d_weight": mod.weight.grad, "d_biases": mod.biases.grad}
    return run


def _cell_run(tag, env):
    from eeg_gnn_ssl_amd import DCGRUCell
    c, dev = cases.cell_inputs(tag, env.adj3d), env.device
    cell = DCGRUCell(c["din"], c["h"], c["k"], 19, filter_type=c["filt"], nonlinearity=c["act"])
    ps.load(cell, c["params"], dev)
    sup, wout = [t.to(dev) for t in c["sup"]], c["wout"].to(dev)

    def run():
        cell.zero_grad(set_to_none=True)
        x, s = c["x"].to(dev).requires_grad_(True), c["s"].to(dev).requires_grad_(True)
        out, _ = cell(sup, x, s)
        (out * wout).sum().backward()
        return {"out": out.detach(), "dx": x.grad, "dh": s.grad, **{"d_" + k: p.grad for k, p in cell.named_parameters()}}
    return run


def _head_run(shape, p_drop, weighted, env):
    from eeg_gnn_ssl_amd import ops
    (b, n, h, c), dev, g = shape, env.device, torch.Generator().manual_seed(77)
    z = torch.randn(b, n, h, generator=g).to(dev)
    w, bias = (0.3 * torch.randn(c, h, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
    y = ((torch.rand(b, generator=g) > 0.5).float() if c == 1 else torch.randint(0, c, (b,), generator=g)).to(dev)
    clip_w = (torch.arange(b) % 3 != 1).float().to(dev) if weighted else None          # (clip 1, 4, .. do not count)
    denom = clip_w.sum().view(1) if weighted else None

    def run():
        w2, b2 = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        state = torch.tensor([4242, 11], dtype=torch.int64, device=dev)
        loss, logits, dz = ops.cls_head_loss(z, w2, b2, y, "detection" if c == 1 else "classification", p_drop, state, clip_w=clip_w, denom=denom)
        return {"loss": loss.detach().reshape(1), "logits": logits, "dz": dz, "dW": w2.grad, "db": b2.grad, "rng": state}
    return run


def _loss_run(kind, weighted, env):
    from eeg_gnn_ssl_amd import ops
    dev, g = env.device, torch.Generator().manual_seed(5)
    if kind in ("bce", "ce"):
        x = torch.randn(37, generator=g) if kind == "bce" else torch.randn(21, 4, generator=g)
        y = (torch.rand(37, generator=g) > 0.5).float() if kind == "bce" else torch.randint(0, 4, (21,), generator=g)
        fn, lead = (ops.bce_with_logits if kind == "bce" else ops.cross_entropy), x.shape[0]
    else:                                         # masked MAE / RMSE: with the scaler at (3, 4, 19, 10); n = 7001: the n % 4 tail path
        name, shape = kind.split("_")
        shape = (7001,) if shape == "7001" else (3, 4, 19, 10)
        scaler = None if len(shape) == 1 else (3.924, 1.56)
        x, y = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        y[torch.rand(shape, generator=g) < 0.2] = 0.0 if scaler is None else -scaler[0] / scaler[1]
        fn = lambda p, t, **kw: ops.masked_regression_loss(p, t, None if scaler is None else scaler[0], None if scaler is None else scaler[1], name, **kw)   # noqa: E731
        lead = shape[0]
    yd = y.to(dev)
    kw = {}
    if weighted:
        clip_w = (torch.arange(lead) % 3 != 1).float().to(dev)
        kw = dict(clip_w=clip_w, denom=clip_w.sum().view(1))

    def run():
        xd = x.clone().to(dev).requires_grad_(True)
        loss = fn(xd, yd, **kw)
        loss.backward()
        return {"loss": loss.detach().reshape(1), "dx": xd.grad}
    return run


def _adam_run(env):
    from eeg_gnn_ssl_amd import ops
    dev, g, n = env.device, torch.Generator().manual_seed(5), 70001
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * s for s in (0.05, 0.001)]      # (second step: no clipping)

    def run():
        p, m, v = p0.to(dev).clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        ws, norm, out = torch.zeros(64, device=dev), torch.zeros(1, device=dev), {}
        for step, gr in enumerate(grads, 1):
            gd = gr.to(dev).clone()
            ops.clip_adam_step(p, gd, m, v, step, 3e-3, (0.9, 0.999), 1e-8, 5e-4, 5.0, 1.0, ws, norm)
            out.update({f"grad{step}": gd, f"norm{step}": norm.clone()})
        return dict(out, p=p, m=m, v=v)
    return run


def _fft_run(window, steps, env, lengths=False):
    from eeg_gnn_ssl_amd import ops
    dev, g = env.device, torch.Generator().manual_seed(2)
    raw = (torch.randn(2, 19, steps * window, generator=g) * 20.0).to(dev)
    perm = torch.stack([torch.arange(19), torch.arange(19)]).to(torch.int32)
    perm[1, [0, 1, 4, 7]] = torch.tensor([1, 0, 7, 4], dtype=torch.int32)
    perm, ls = perm.to(dev), torch.tensor([0.0, float(np.log(1.137))]).to(dev)
    ln = torch.tensor([steps, 1], dtype=torch.int64, device=dev) if lengths else None

    def run():
        fr, fs = ops.fft_features(raw, window=window, mean=0.5, std=2.0, perm=perm, log_scale=ls, lengths=ln, padding_val=0.25)
        return {"feat_raw": fr, "feat_std": fs, "raw_only": ops.fft_features(raw, window=window)[0]}
    return run


def _corr_run(shape, top_k, env):
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(*shape, generator=g)
    xs[0, :, 3, :] = 0.0                          # a silent electrode
    xd = xs.to(env.device)

    def run():
        (s1, s2), adj = ops.correlation_supports(xd, top_k=top_k, return_adj=True)
        return {"s1": s1, "s2": s2, "adj": adj}
    return run


def _hop_polys_run(filt, batched, env):
    sup = [s.to(env.device) for s in cases.supports_for(filt, env.adj3d, 3, batched)]
    return lambda: {"P": torch.ops.eeg_dcrnn.hop_polys(sup, 2, 3)}


def _spectral_pack_run(n, fin, env):
    g = torch.Generator().manual_seed(5)
    s2 = ps.shared_laplacian(n, env.adj3d, g).to(env.device)
    h, m = 64, 3
    kdim = (fin + h) * m
    wg, wc = (torch.randn(kdim, 2 * h, generator=g) / kdim ** 0.5).to(env.device), (torch.randn(kdim, h, generator=g) / kdim ** 0.5).to(env.device)

    def run():
        basis = torch.ops.eeg_dcrnn.spectral_basis(s2)
        return {"basis": basis, "spack": torch.ops.eeg_dcrnn.pack_cell_spectral(wg, wc, basis, fin, h, m, n)}
    return run


OPERATOR_CASES = {
    "dconv_lap_small": lambda env: _dconv_run("lap_small", env),
    "dconv_lap_small_unbatched": lambda env: _dconv_run("lap_small_unbatched", env),
    "dconv_dual_small": lambda env: _dconv_run("dual_small", env),
    "cell_lap_small": lambda env: _cell_run("lap_small", env),
    "cell_dual_small": lambda env: _cell_run("dual_small", env),
    "cell_lap_small_relu": lambda env: _cell_run("lap_small_relu", env),
    "head_loss_b1_c1": lambda env: _head_run((1, 19, 64, 1), 0.0, False, env),
    "head_loss_b5_c4_dropout": lambda env: _head_run((5, 19, 64, 4), 0.5, False, env),
    "head_loss_b37_n21_h32": lambda env: _head_run((37, 21, 32, 3), 0.0, False, env),
    "head_loss_w_b5_c4": lambda env: _head_run((5, 19, 64, 4), 0.0, True, env),
    "head_loss_w_b5_c1_dropout": lambda env: _head_run((5, 19, 64, 1), 0.5, True, env),
    "loss_bce": lambda env: _loss_run("bce", False, env),
    "loss_ce": lambda env: _loss_run("ce", False, env),
    "loss_bce_w": lambda env: _loss_run("bce", True, env),
    "loss_ce_w": lambda env: _loss_run("ce", True, env),
    "loss_masked_mae": lambda env: _loss_run("mae_small", False, env),
    "loss_masked_rmse": lambda env: _loss_run("rmse_small", False, env),
    "loss_masked_mae_w": lambda env: _loss_run("mae_small", True, env),
    "loss_masked_mae_n7001": lambda env: _loss_run("mae_7001", False, env),
    "loss_masked_rmse_n7001": lambda env: _loss_run("rmse_7001", False, env),
    "clip_adam_step": _adam_run,
    "fft_w200": lambda env: _fft_run(200, 5, env),
    "fft_w200_lengths": lambda env: _fft_run(200, 5, env, lengths=True),
    "fft_w40": lambda env: _fft_run(40, 3, env),
    "fft_w252": lambda env: _fft_run(252, 2, env),
    "corr_supports_d100": lambda env: _corr_run((5, 7, 19, 100), 3, env),
    "corr_supports_d8_t1": lambda env: _corr_run((2, 1, 19, 8), 2, env),
    "corr_supports_d200": lambda env: _corr_run((2, 3, 19, 200), 3, env),
    "hop_polys_dual": lambda env: _hop_polys_run("dual_random_walk", True, env),
    "hop_polys_lap_shared": lambda env: _hop_polys_run("laplacian", False, env),
    "spectral_pack_n19_fin100": lambda env: _spectral_pack_run(19, 100, env),
    "spectral_pack_n20_fin64": lambda env: _spectral_pack_run(20, 64, env),
}


def check_operator_case(name, env, patch=None, record=None):
    t0, what = time.perf_counter(), f"operator {name}"
    run = OPERATOR_CASES[name](env)
    clean = run() if env.emu else check_repeat(run, what)
    stats = check_poison(run, what, patch, clean, need_calls=name != "clip_adam_step")      # (the optimiser tail works in its caller's buffers)
    if record is not None:
        record.append(dict(case=what, checks=["b"] if env.emu else ["a", "b"], stats=stats, seconds=time.perf_counter() - t0, verdict="pass"))


# ---- TrainStep: two eager steps, clean against poisoned from construction on -------------------------------------------------------------
TRAIN_MODES = ("detection", "classification", "ssl")
TRAIN_B, TRAIN_T, TRAIN_TY = 4, 3, 2


def _train_case(mode, env):
    """-> (make(): a fresh TrainStep, the two batches).  detection: features on 19 nodes, the 2-D distance graph (spectral form);
    classification: raw signals, per-clip correlation graphs, variable lengths; ssl: the raw pair, 16 features per step -- a decoder the
    persistent kernels take"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, ops, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    dev, g, n, b, t = env.device, torch.Generator().manual_seed(21), 19, TRAIN_B, TRAIN_T
    if mode == "detection":
        cfg = orc.DCRNNConfig(filter_type="laplacian", input_dim=8, num_classes=1, rnn_units=64)
        xs, ys, lens = torch.randn(2, b, t, n, 8, generator=g), torch.randint(0, 2, (2, b), generator=g).float(), torch.full((2, b), t)
        supports, kind, kw = [s.to(dev) for s in utils.compute_supports(env.adj3d, "laplacian")], "classification", {}
    elif mode == "classification":
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=4, num_classes=4, rnn_units=16)
        xs, ys, lens = torch.randn(2, b, n, t * 8, generator=g), torch.randint(0, 4, (2, b), generator=g), torch.randint(1, t + 1, (2, b), generator=g)
        supports, kind, kw = None, "classification", dict(raw_window=8, raw_mean=0.3, raw_std=1.7, padding_val=0.0)
    else:
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=16, output_dim=16, rnn_units=64)
        xs, ys, lens = torch.randn(2, b, n, t * 32, generator=g), torch.randn(2, b, n, TRAIN_TY * 32, generator=g), None
        supports, kind, kw = None, "ssl", dict(raw_window=32, raw_mean=0.3, raw_std=1.7, data_augment=True)
        m = 2 * cfg.max_diffusion_step + 1
        assert ops.decoder_is_persistent(TRAIN_TY, b, n, 64, 16, m, cfg.num_rnn_layers), "the SSL case is there for the persistent decoder"
    params = orc.init_params(cfg, kind, seed=6)
    task = mode

    def make():
        model = DCRNNModel_nextTimePred(ps.make_args(cfg), device=dev) if mode == "ssl" else DCRNNModel_classification(ps.make_args(cfg), cfg.num_classes, device=dev)
        ps.load(model, params, dev)
        model.train()
        torch.manual_seed(99)                                       # the seed of the step's augmentation generator
        return TrainStep(model, task=task, **kw)

    batches = [(xs[i].to(dev), ys[i].to(dev), None if lens is None else lens[i].to(dev), supports) for i in range(2)]
    return make, batches


def train_run(mode, env):
    make, batches = _train_case(mode, env)
    st = make()
    losses = [st.step(*bt).detach().clone().reshape(1) for bt in batches]
    return {"loss1": losses[0], "loss2": losses[1], "parameters": st.fp.flat.detach().clone(), "exp_avg": st.exp_avg.clone(), "exp_avg_sq": st.exp_avg_sq.clone()}


def check_train_step(mode, env, patch=None, record=None):
    t0, what = time.perf_counter(), f"TrainStep {mode}"
    clean = train_run(mode, env)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values()), f"{what}: the clean run is not finite"
    stats = None
    for label, fill in FILLS.items():
        with poison(fill, patch) as st:
            got = train_run(mode, env)
        assert st["calls"] > 0 and st["floats"] > 0
        stats = stats or dict(st)
        assert_same(got, clean, f"{what}: constructed and stepped twice with allocations filled with {label} against clean")
    if record is not None:
        record.append(dict(case=what, checks=["b"], stats=stats, seconds=time.perf_counter() - t0, verdict="pass"))


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def format_record(record, device):
    lines = [f"invariance suite on {'the MI355X' if device == 'cuda' else 'the emulator'}: a = {REPEATS} bit-identical repeats, b = allocations poisoned "
             f"({' / '.join(FILLS)}), c = dirty neighbour, d = clip isolation",
             f"{'case':<52}{'checks':<28}{'verdict':<12}{'poisoned allocations':>22}{'floats':>14}{'seconds':>9}"]
    for r in record:
        lines.append(f"{r['case']:<52}{' '.join(r['checks']):<28}{r['verdict']:<12}{r['stats']['calls']:>22}{r['stats']['floats']:>14}{r['seconds']:>9.2f}")
    lines.append(f"{len(record)} cases, {sum(r['verdict'] == 'pass' for r in record)} pass, {sum(r['seconds'] for r in record):.1f} s")
    return lines


def main(argv):
    import argparse
    import tempfile
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[-1])
    ap.add_argument("--device", choices=("cuda", "cpu"), required=True)
    ap.add_argument("--out")
    ap.add_argument("--tables", nargs="*", default=list(TABLES) + ["operators", "train"])
    a = ap.parse_args(argv)
    torch.set_num_threads(16)
    adj3d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adj_mx_3d.npy"))
    set_knob = None
    if a.device == "cpu":
        import emu_support
        lib = emu_support.install_emulator()
        set_knob = lambda key, value: lib.call("eeg_dcrnn_set_tuning", key, value)      # noqa: E731
    record, failed = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        env = Env(a.device, adj3d, set_knob, qg.build_plan_driver(tmp))
        jobs = [(check_table_case, (t, n)) for t in TABLES if t in a.tables for n in table_cases(t, env.emu)]
        jobs += [(check_operator_case, (n,)) for n in OPERATOR_CASES if "operators" in a.tables]
        jobs += [(check_train_step, (m,)) for m in TRAIN_MODES if "train" in a.tables]
        for fn, args in jobs:
            done = len(record)
            try:
                fn(*args, env, record=record)
            except AssertionError as e:
                failed += 1
                if len(record) == done:
                    record.append(dict(case=" ".join(args), checks=[], stats={"calls": 0, "floats": 0}, seconds=0.0, verdict="FAIL"))
                print(f"FAILED {' '.join(args)}: {e}", flush=True)
            print(format_record(record[-1:], a.device)[-2], flush=True)
    lines = format_record(record, a.device)
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
