"""Results depend on inputs only (tests/invariance_suite.py): every case of the five instance tables run 8 times bit-identically, with
every allocation of the operator layer poisoned (`monkeypatch.setattr(ops, "_new", ...)`: quiet NaN and 7.0e3, floating-point tensors
only), after a dirtier neighbour, and with the other clips' inputs replaced; the operators of the training tail, the feature and graph
front end likewise; `TrainStep` constructed and stepped under the poison.  The repeat and neighbour checks need the MI355X (`-m gpu`);
poison and clip isolation also run on the emulator build of the kernel sources, on the tables' emulator share.  Two tests prove that
the harness bites: a layer whose `eeg_dcrnn_zero` call is filtered out fails the poison check by name, and a changed kept clip fails
the isolation check."""
import os

import pytest
import torch

import dec_kernel_suite as dk
import diffuse_corr_suite as dc
import invariance_suite as iv
import quad_gemm_suite as qg
import seq_kernel_suite as sk
import spec_plan_suite as sp


@pytest.fixture
def emulator():
    import emu_support
    lib = emu_support.install_emulator()
    yield lib
    emu_support.uninstall()


@pytest.fixture
def hip_library():
    from eeg_gnn_ssl_amd import _lib
    _lib._LIB = None
    lib = _lib.get_lib()                  # ImportError if the HIP library is missing: no fallback
    assert lib.is_device_build and os.path.basename(lib.path) == "libeeg_dcrnn_hip.so"
    assert torch.cuda.is_available()
    yield lib


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


@pytest.fixture
def emu_env(emulator, adj3d, plan_driver):
    return iv.Env("cpu", adj3d, lambda key, value: emulator.call("eeg_dcrnn_set_tuning", key, value), plan_driver)


@pytest.fixture
def gpu_env(hip_library, adj3d):
    return iv.Env("cuda", adj3d)


def _params(emu):
    return [pytest.param(t, n, id=f"{t}-{n}") for t in iv.TABLES for n in iv.table_cases(t, emu)]


# ---- no device: the parametrisation against the tables ------------------------------------------------------------------------------
def test_invariance_covers_every_case_of_the_tables():
    """the MI355X parametrisation is each table's whole case set, the emulator's is each table's emulator share: a case added to a table
    later is under the invariance checks without a line here"""
    gpu = {t: {p.values[1] for p in _params(False) if p.values[0] == t} for t in iv.TABLES}
    assert gpu == {"seq": set(sk.CASES), "quad": set(qg.CASES), "dec": set(dk.ALL_CASES), "spec": set(sp.PRODUCT_CASES),
                   "diffuse": set(dc.DIFFUSE_CASES), "corr": set(dc.CORR_CASES)}
    emu = {t: {p.values[1] for p in _params(True) if p.values[0] == t} for t in iv.TABLES}
    assert emu == {"seq": set(sk.EMU_CASES) | set(sk.KNOB_CASES), "quad": set(qg.CASES), "dec": set(dk.EMU_CASES), "spec": set(sp.CASES),
                   "diffuse": set(dc.DIFFUSE_CASES), "corr": set(dc.CORR_CASES)}
    # clip isolation: every walk case, and every kernel template of the recurrent kernels through a case of its own
    for emu_share in (False, True):
        seq = iv.isolation_cases("seq", emu_share)
        want = {sk.template_of(s) for n in iv.table_cases("seq", emu_share) for s in (iv._seq_case(n)[3] or iv._seq_case(n)[1]["expect"]).values()}
        assert {sk.template_of(s) for n in seq if not n.endswith("_walk") for s in (iv._seq_case(n)[3] or iv._seq_case(n)[1]["expect"]).values()} == want
    assert set(sk.WALK_CASES) <= set(iv.isolation_cases("seq", False)) and set(dk.WALK_CASES) <= set(iv.isolation_cases("dec", False))
    assert len(set(iv.isolation_cases("dec", False)) - set(dk.WALK_CASES)) == 4          # CX0 = 12, 16, 20 and the per-step path
    # the dirtier cases are cases of their tables
    assert iv.DIRTIER["seq"] in sk.CASES and iv.DIRTIER["dec"] in dk.CASES and iv.DIRTIER["spec"] in sp.PRODUCT_CASES
    assert sk.CASES[iv.DIRTIER["seq"]]["expect"]["seq_bwd"] == sk.bwd1(64, 7, 5) and dk.cx0_of(dk.CASES[iv.DIRTIER["dec"]]["dout"]) == 20


def test_kept_clips():
    assert iv.kept_clips(257) == [0, 128, 256] and iv.kept_clips(4) == [0, 2, 3] and iv.kept_clips(3) == [0, 2] and iv.kept_clips(2) == [0]


# ---- emulator: poison, clip isolation, the case's own check inside the NaN context ---------------------------------------------------
@pytest.mark.parametrize("table, name", _params(True))
def test_table_case_emu(emu_env, monkeypatch, table, name):
    row = iv.check_table_case(table, name, emu_env, monkeypatch)
    assert "b" in row["checks"] and ("d" in row["checks"]) == (name in iv.isolation_cases(table, True))


@pytest.mark.parametrize("name", list(iv.OPERATOR_CASES))
def test_operator_emu(emu_env, monkeypatch, name):
    iv.check_operator_case(name, emu_env, monkeypatch)


@pytest.mark.parametrize("mode", iv.TRAIN_MODES)
def test_train_step_emu(emu_env, monkeypatch, mode):
    iv.check_train_step(mode, emu_env, monkeypatch)


def _zero_call_bite(env, lib, monkeypatch):
    run = iv.second_layer_runner(env.device)
    stats = iv.check_poison(run, "second layer", monkeypatch)                   # as it is: slot 0 of dX is zeroed, nothing moves
    assert stats["calls"] > 0 and not run()["dX"][0].any()
    with iv.without_entry(lib, "eeg_dcrnn_zero"):
        with pytest.raises(AssertionError, match=r"differ in .*dX"):
            iv.check_poison(run, "second layer without its eeg_dcrnn_zero call", monkeypatch)
    iv.check_poison(run, "second layer", monkeypatch)                           # (the filter is gone)


def _isolation_bite(env):
    name = "h16_m3_n19"                                                         # 4 clips of 2 steps: clips 0, 2, 3 are kept
    assert iv.check_isolation("seq", name, env) == [0, 2, 3]
    with pytest.raises(AssertionError, match=r"differ in .*hseq"):
        iv.check_isolation("seq", name, env, tamper=True)


def test_poison_check_bites_without_the_zero_call_emu(emu_env, emulator, monkeypatch):
    _zero_call_bite(emu_env, emulator, monkeypatch)


def test_isolation_check_bites_on_a_changed_kept_clip_emu(emu_env):
    _isolation_bite(emu_env)


# ---- MI355X: repeat, poison, dirty neighbour, clip isolation -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("table, name", _params(False))
def test_table_case(gpu_env, monkeypatch, table, name):
    row = iv.check_table_case(table, name, gpu_env, monkeypatch)
    assert row["checks"][:2] == ["a", "b"] and ("c" in row["checks"]) == (table in iv.DIRTIER)
    assert ("d" in row["checks"]) == (name in iv.isolation_cases(table, False))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(iv.OPERATOR_CASES))
def test_operator(gpu_env, monkeypatch, name):
    iv.check_operator_case(name, gpu_env, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", iv.TRAIN_MODES)
def test_train_step(gpu_env, monkeypatch, mode):
    iv.check_train_step(mode, gpu_env, monkeypatch)


@pytest.mark.gpu
def test_poison_check_bites_without_the_zero_call(gpu_env, hip_library, monkeypatch):
    _zero_call_bite(gpu_env, hip_library, monkeypatch)


@pytest.mark.gpu
def test_isolation_check_bites_on_a_changed_kept_clip(gpu_env):
    _isolation_bite(gpu_env)
