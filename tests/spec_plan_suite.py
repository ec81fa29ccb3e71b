"""The kernels of the spectral form (csrc/kernels_spectral.h, kernels_gemm_g.h, kernels_gemm_f.h) at every template instance the launch
plans of csrc/spec_launch.h can hand a layer.  Which of them takes a shape is invisible to a parity test -- the fallbacks give the same
numbers -- so every case here is one small model through `parity_suite.check_spectral_form` (logits and all gradients against the oracle
and against the general path) with the event recorder on, and the kernel symbol recorded per launch role must be the planned one.  The
plan driver of tests/emu says, without a GPU, what a layer is planned with and which instances are reachable at all; CASES must cover
exactly that set.  These kernels have no row threshold, so the smallest shapes do: T = 3 steps of 4 or 5 clips, S = 12 or 15 rows per
frequency -- not a multiple of 16, so pad rows exist.  Run by tests/test_spec_plans.py on the MI355X library (the cases without dev
knobs: they are compile-time zeros there) and by tests/test_emu_parity.py on the emulator (all of them)."""
import subprocess

import parity_suite as ps
import quad_gemm_suite as qg

NO_KNOBS = (0, 0, 0)                  # dev keys 20 (x-part NN grouped), 23 (weight gradients as grouped launches), 17 (dX as two passes)
KNOB_KEYS = (20, 23, 17)
T_LEN = 3
EMU_CUS = qg.EMU_CUS


# ---- kernel symbols as the event recorder spells them ---------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def nnf(kq, swz=False):
    return f"gemm_nnf_kernel<{kq}, {_b(swz)}>"


def nng(nj):
    return f"gemm_nng_kernel<{nj}, 2>"


def tnf(fxt):
    return f"gemm_tnf_kernel<{fxt}>"


def tng(kt, planar=False):
    return f"gemm_tnq_grouped_kernel<{kt}, 6, 16, {_b(planar)}>"


TNG_PAIR = "gemm_tnq_grouped_pair_kernel<2, 16, true>"


def dxf(nt):
    return f"gemm_dxf_kernel<{nt}>"


def mix_mfma(direction, ks):
    return f"spec_mix_mfma_kernel<{direction}, {ks}>"


MIX_IN19, MIX_GENERIC = "spec_mix_in_kernel<19>", "spec_mix_generic_kernel"
FAMILY = ("gemm_nnf_kernel", "gemm_nng_kernel", "gemm_tnf_kernel", "gemm_tnq_grouped_kernel", "gemm_tnq_grouped_pair_kernel", "gemm_dxf_kernel",
          "spec_mix_mfma_kernel", "spec_mix_in_kernel", "spec_mix_out_kernel", "spec_mix_generic_kernel")
ROLES = ("gemm_nn_xw", "gemm_tn_f", "gemm_tn_x", "gemm_tn_h", "gemm_dx_f", "gemm_nn_dx", "spec_mix_x", "spec_mix_y", "spec_mix_h", "spec_mix_dy",
         "spec_mix_dx")


def is_spectral(symbol):
    return symbol.split("<")[0] in FAMILY


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# n nodes, din input features, 2 layers (layer 0: Fin = din, no dX; layer 1: Fin = 64 with dX), b clips, dev knobs.  expect: role -> the
# symbols that MUST be recorded under it (one per layer that launches the role; layer 0 first).
CASES = {
    # the EEG montage at the width of the FFT features: K = 100 is 25 sixteen-byte units (odd: plain image), layer 1 the swizzled K = 64
    "n19_din100": dict(n=19, din=100, b=4, knobs=NO_KNOBS,
                       expect={"gemm_nn_xw": {nnf(13), nnf(8, True)}, "gemm_tn_f": {tnf(4), tnf(2)}, "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    # the other three register-weight depths and Xh tile counts
    "n19_din36": dict(n=19, din=36, b=5, knobs=NO_KNOBS,
                      expect={"gemm_nn_xw": {nnf(5), nnf(8, True)}, "gemm_tn_f": {tnf(2)}, "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    "n19_din68": dict(n=19, din=68, b=4, knobs=NO_KNOBS,
                      expect={"gemm_nn_xw": {nnf(9), nnf(8, True)}, "gemm_tn_f": {tnf(3), tnf(2)}, "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    "n19_din12": dict(n=19, din=12, b=5, knobs=NO_KNOBS,
                      expect={"gemm_nn_xw": {nnf(2), nnf(8, True)}, "gemm_tn_f": {tnf(1), tnf(2)}, "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    # one past the fused weight-gradient kernel's widest input: the grouped launches (one 160-wide k-block) and -- 33 units per row, but
    # no instance 17 deep -- the grouped NN kernel
    "n19_din132": dict(n=19, din=132, b=4, knobs=NO_KNOBS,
                       expect={"gemm_nn_xw": {nng(3), nnf(8, True)}, "gemm_tn_x": {tng(5)}, "gemm_tn_h": {TNG_PAIR}, "gemm_tn_f": {tnf(2)},
                               "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    # the time-domain width: two 128-wide k-blocks, 50 units per row (even)
    "n19_din200": dict(n=19, din=200, b=5, knobs=NO_KNOBS,
                       expect={"gemm_nn_xw": {nng(3), nnf(8, True)}, "gemm_tn_x": {tng(4)}, "gemm_tn_h": {TNG_PAIR}, "gemm_tn_f": {tnf(2)},
                               "gemm_dx_f": {dxf(19)}, "spec_mix_x": {MIX_IN19}}),
    # 20 nodes: the last count of the fused dX kernel (node count at run time) and of the 10-step MFMA mix
    "n20_din64": dict(n=20, din=64, b=4, knobs=NO_KNOBS,
                      expect={"gemm_nn_xw": {nnf(8, True)}, "gemm_tn_f": {tnf(2)}, "gemm_dx_f": {dxf(0)}, "spec_mix_x": {mix_mfma(0, 10)}}),
    # 24 nodes: dX as the grouped GEMM + the node mix back, 16-step MFMA mixes
    "n24_din64": dict(n=24, din=64, b=5, knobs=NO_KNOBS,
                      expect={"gemm_nn_xw": {nnf(8, True)}, "gemm_tn_f": {tnf(2)}, "gemm_nn_dx": {nng(1)}, "spec_mix_dx": {mix_mfma(1, 16)},
                              "spec_mix_x": {mix_mfma(0, 16)}}),
    # another montage at a width that is not whole 128-byte tiles: the generic mix; 5 units per row but no instance 3 deep
    "n5_din20": dict(n=5, din=20, b=4, knobs=NO_KNOBS,
                     expect={"gemm_nn_xw": {nng(3), nnf(8, True)}, "gemm_tn_f": {tnf(1), tnf(2)}, "gemm_dx_f": {dxf(0)}, "spec_mix_x": {MIX_GENERIC}}),
    # the three dev knobs (development builds and the emulator): the round-5 kernels at the widths the fused ones took over -- the planar
    # grouped TN instance is reachable only this way
    "n20_din64_knobs": dict(n=20, din=64, b=5, knobs=(1, 1, 1),
                            expect={"gemm_nn_xw": {nng(3)}, "gemm_tn_x": {tng(2, True)}, "gemm_tn_h": {TNG_PAIR}, "gemm_nn_dx": {nng(1)},
                                    "spec_mix_dx": {mix_mfma(1, 10)}, "spec_mix_x": {mix_mfma(0, 10)}}),
}
PRODUCT_CASES = tuple(name for name, case in CASES.items() if case["knobs"] == NO_KNOBS)


# ---- what a model plans: the calls of csrc/api.cpp restated, answered by the plan driver ------------------------------------------
def spec_rows(s):
    return (s + 15) // 16 * 16


def layer_calls(n, t, b, fin, need_dx, cus, knobs):
    """driver lines of one spectral layer, as layer_fwd / layer_bwd / bwd_ws of api.cpp build their calls -> [(role, line, must)]: must =
    the role is launched whatever the recurrent kernels do (the other mixes run only where the two-wave kernels do not mix themselves)"""
    sp, kn = spec_rows(t * b), " ".join(str(k) for k in knobs)
    calls = [("gemm_nn_xw", f"snn {fin} {sp} {n} 12 {cus} {kn}", True),
             ("tn", f"stn {fin} 64 {sp} {n} {cus} {kn}", True),
             ("spec_mix_x", f"mix 1 {n} {t} {b} {fin} 0", not need_dx),          # (a layer above the first may be handed U^T h)
             ("spec_mix_y", f"mix 0 {n} {t} {b} 192 0", False),
             ("spec_mix_h", f"mix 1 {n} {t + 1} {b} 64 {b + sp}", False),
             ("spec_mix_h", f"mix 1 {n} {t} {b} 64 0", False),
             ("spec_mix_dy", f"mix 1 {n} {t} {b} 192 0", False)]
    if need_dx:
        calls.append(("dx", f"sdx {fin} {n} {t} {b} {cus} {kn}", True))
    return calls


def _launches(line):
    """a spectral plan line of the driver -> the kernel symbols of its launches"""
    assert not line.startswith("error"), line
    return [f for f in line.split(" ; ") if is_spectral(f)]


def planned(exe, models):
    """models: list of (n, din, layers, t, b, cus, knobs) -> per model (must, may): role -> set of symbols"""
    lines, index = [], []
    for i, (n, din, layers, t, b, cus, knobs) in enumerate(models):
        for lay in range(layers):
            for role, line, must in layer_calls(n, t, b, din if lay == 0 else 64, lay > 0, cus, knobs):
                lines.append(line)
                index.append((i, role, must))
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    res = [({}, {}) for _ in models]
    for (i, role, must), line in zip(index, out):
        syms = _launches(line)
        if role == "tn":
            named = {"gemm_tn_f": syms} if len(syms) == 1 else {"gemm_tn_x": syms[:1], "gemm_tn_h": syms[1:]}
        elif role == "dx":
            named = {"gemm_dx_f": syms} if len(syms) == 1 else {"gemm_nn_dx": syms[:1], "spec_mix_dx": syms[1:]}
        else:
            named = {role: syms}
        for r, s in named.items():
            res[i][0 if must else 1].setdefault(r, set()).update(s)
    return res


def supported(exe, shapes):
    """shapes: list of (t, b, n, fin, need_dx) -> list of bool (spec_supported at 64 units, 3 hop matrices)"""
    lines = [f"sup {t} {b} {n} 64 {fin} 3 {dx}" for t, b, n, fin, dx in shapes]
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(lines)
    return [o == "1" for o in out]


def reachable_instances(exe, cus=256):
    """every kernel symbol some supported two-layer model is planned with: 2 .. 32 nodes, every input width up to 264 and the widest
    ones, without knobs, with each knob alone and with all three"""
    widths = list(range(4, 268, 4)) + [512, 1020, 1024]
    shapes = [(n, din) for n in range(2, 33) for din in widths]
    ok = supported(exe, [(T_LEN, 4, n, din, 0) for n, din in shapes])
    models = [(n, din, 2, T_LEN, 4, cus, kn) for (n, din), good in zip(shapes, ok) if good
              for kn in (NO_KNOBS, (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))]
    return {s for must, may in planned(exe, models) for roles in (must, may) for syms in roles.values() for s in syms}


# ---- the model under test -------------------------------------------------------------------------------------------------------
SEED = 21


def run_model(name, device, adj3d, x_scale=1.0):
    """-> run(): one forward + backward of the case's model in the spectral form (operands of check_case; dev knobs are the caller's to
    set) -> (logits, {parameter name: gradient}).  x_scale: the clips scaled"""
    case = CASES[name]
    c = ps.spectral_form_operands(adj3d, din=case["din"], layers=2, t_len=T_LEN, b=case["b"], classes=1, n=case["n"], seed=SEED)
    return ps.run_spectral_form(device, c, c.x * x_scale if x_scale != 1.0 else None)


def check_case(name, device, adj3d, exe, cus, set_knob=None):
    """One case: check_spectral_form with the recorder on; per role the spectral-family symbols recorded (the general-path comparison inside
    the check launches other kernels under some of the same roles) against the plan.  set_knob(key, value): sets a dev knob."""
    case = CASES[name]
    must, may = planned(exe, [(case["n"], case["din"], 2, T_LEN, case["b"], cus, case["knobs"])])[0]
    assert must == {r: set(s) for r, s in case["expect"].items()}, (name, must)
    assert case["knobs"] == NO_KNOBS or set_knob is not None, "dev knobs need a development build"
    try:
        for key, value in zip(KNOB_KEYS, case["knobs"]):
            if value:
                set_knob(key, value)
        ran = ps.kernels_run(lambda: ps.check_spectral_form(device, adj3d, din=case["din"], layers=2, t_len=T_LEN, b=case["b"], classes=1,
                                                            n=case["n"], seed=SEED))
    finally:
        for key, value in zip(KNOB_KEYS, case["knobs"]):
            if value:
                set_knob(key, 0)
    got = {role: {s for s in ran.get(role, {}) if is_spectral(s)} for role in ROLES}
    print(f"spec-plan {name} ran: " + "; ".join(f"{role} = {', '.join(sorted(s))}" for role, s in got.items() if s))
    for role in ROLES:
        lo, hi = must.get(role, set()), must.get(role, set()) | may.get(role, set())
        assert lo <= got[role] <= hi, f"{name}: {role} ran {sorted(got[role])}, planned {sorted(lo)} (and where the recurrent kernels do not mix: {sorted(hi - lo)})"
    return got
