"""Gates, losses and the head at saturation, ties and exact zeros (tests/range_suite.py): the recurrent and decoder kernels with biases
of up to +-1e4 on their gates and candidates, the three copies of the BCE / cross-entropy arithmetic at |logit| up to 1e4 against float64,
the masked loss where its code branches, and the head's arg-max at exact ties and exact zeros.  Every check runs on the emulator build
of the kernel sources (which substitutes expf and 1 / x for the hardware's exp2 and reciprocal: the emulator pins the arithmetic around
them, the MI355X runs the hardware forms) and again, marked `gpu`, on the MI355X library."""
import os

import pytest
import torch

import dec_kernel_suite as dk
import range_suite as rs
import seq_kernel_suite as sk


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
    torch.set_num_threads(16)             # (the float64 references: a fraction of a second per case)
    yield lib


# ---- no GPU: the tables ------------------------------------------------------------------------------------------------------------
def test_band_table_crosses_both_overflow_thresholds():
    """tanh is 1 - 2 rcp(1 + exp2(2x log2 e)): exp2 overflows from 2x log2 e = 128, x = 44.4; sigmoid is rcp(1 + exp2(-x log2 e)): from
    x = 88.7.  Every band sits on every kind of unit of a 16-unit layer already: reset gate, update gate (rolled by 5), candidate (by 9)."""
    mags = sorted({abs(v) for v in rs.BANDS})
    assert mags == [0.0, 8.0, 20.0, 45.0, 90.0, 200.0, 1e4] and len(rs.BANDS) == 13 and sum(rs.BANDS) == 0
    assert max(m for m in mags if m < 44.4) == 20.0 and min(m for m in mags if m > 44.4) == 45.0
    assert max(m for m in mags if m < 88.7) == 45.0 and min(m for m in mags if m > 88.7) == 90.0
    assert rs.band(64)[:13].tolist() == list(rs.BANDS) and rs.band(64)[13] == rs.BANDS[0]
    for h in (16, 32, 64):
        g = rs.gate_band(h)
        assert g.shape == (2 * h,) and torch.equal(g[h:], g[:h].roll(5)) and torch.equal(rs.cand_band(h), g[:h].roll(9))
        assert {abs(v) for v in g[:h].tolist()} == set(mags) or h == 16      # (16 units: every band but one of the last three)
    op = rs.layer_operands(sk.CASES["h64_m5_n20"])                           # relu: the candidate bias stays well scaled
    assert float(op["bc"].abs().max()) < 1.0 and float(op["bg"].abs().max()) > 9e3
    assert float(rs.layer_operands(sk.CASES["h64_m3_n19"])["bc"].abs().max()) > 9e3


def test_case_tables_name_one_case_per_kernel_template_with_an_activation():
    templates = {sk.template_of(s) for name in rs.LAYER_CASES for s in sk.CASES[name]["expect"].values()}
    assert templates == {sk.template_of(s) for c in sk.CASES.values() for s in c["expect"].values()}
    emu = {sk.template_of(s) for name in rs.EMU_LAYER_CASES for s in sk.CASES[name]["expect"].values()}
    emu |= {sk.template_of(s) for name in rs.EMU_KNOB_LAYER_CASES for s in sk.KNOB_CASES[name][2].values()}
    assert emu == templates
    assert all(sk.CASES[name]["b"] <= 5 for name in rs.EMU_LAYER_CASES)
    acts = {sk.CASES[name]["act"] for name in rs.LAYER_CASES}
    assert acts == {"tanh", "relu"} and {sk.CASES[name]["n"] for name in rs.LAYER_CASES} >= {19, 20}
    # decoder: narrow tanh cases, and one whose first layer is wider than 128 outputs (the wide backward: CX0 = 16)
    assert any(dk.CASES[n]["act"] == "tanh" and dk.CASES[n]["dout"] <= 128 for n in rs.DEC_CASES)
    assert any(dk.CASES[n]["dout"] > 128 and dk.cx0_of(dk.CASES[n]["dout"]) == 16 for n in rs.DEC_CASES)
    assert set(rs.EMU_DEC_CASES) <= set(rs.DEC_CASES) and set(rs.EMU_LAYER_CASES) <= set(rs.LAYER_CASES)


def test_criterion_sets_hold_the_logits_and_rows_they_are_there_for():
    x, y = rs.bce_set()
    assert x.numel() == 69 and sorted(set(y.tolist())) == [0.0, 0.30000001192092896, 1.0]
    assert {abs(v) for v in x.tolist()} == {float(torch.tensor(v)) for v in (0, 1e-8, 1e-3, 1, 16.5, 17.5, 20, 87, 88.5, 89.5, 104, 1e4)}
    assert rs.bce_set(5)[0].numel() == 345 > 256
    for c in (2, 4, 7):
        rows, t = rs.ce_set(c)
        assert rows.shape[1] == c and float(rows.abs().max()) == 1e4
        equal = (rows == rows[:, :1]).all(1)
        assert equal.any() and set(t[equal].tolist()) == {0, c - 1}
        spread = rows.max(1).values - rows.min(1).values
        assert (spread == 100).any() and (spread >= 1e4).any()
        pick = rows.gather(1, t.view(-1, 1)).view(-1)
        assert (pick[~equal] == rows[~equal].max(1).values).any() and (pick[~equal] == rows[~equal].min(1).values).any()
        assert rs.ce_set(c, 14)[0].shape[0] > 256
    for form in ("clip_w", "clip_u"):
        for b in (69, 345):
            u = rs.clip_weights_for(form, b, True)[0]
            assert (u == 0).any() and (u != 0).any()
            for k in range(3):                               # every weight meets every target of the BCE set
                assert len(set(u[k::3].tolist())) == (2 if form == "clip_w" else 3)
    assert set(rs.clip_weights_for("clip_u", 69, True)[0].tolist()) == {0.0, 0.5, 3.0}


# ---- emulator --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rs.EMU_LAYER_CASES))
def test_banded_layer_emu(emulator, name):
    rs.check_layer(name, "cpu")


@pytest.mark.parametrize("name", list(rs.EMU_KNOB_LAYER_CASES))
def test_banded_layer_under_dev_knobs_emu(emulator, name):
    base, knobs, expect = sk.KNOB_CASES[name]
    for key, value in knobs.items():
        emulator.call("eeg_dcrnn_set_tuning", key, value)
    try:
        rs.check_layer(base, "cpu", expect=expect)
    finally:
        for key in knobs:
            emulator.call("eeg_dcrnn_set_tuning", key, 0)


@pytest.mark.parametrize("name", list(rs.EMU_DEC_CASES))
def test_banded_decoder_emu(emulator, name):
    rs.check_decoder(name, "cpu")


def test_bce_emu(emulator):
    rs.check_bce("cpu")


def test_ce_emu(emulator):
    rs.check_ce("cpu")


def test_head_criteria_emu(emulator):
    rs.check_head_criteria("cpu")


def test_eval_scores_emu(emulator):
    rs.check_eval_scores("cpu")


def test_masked_loss_edges_emu(emulator):
    rs.check_masked_loss_edges("cpu")


def test_head_ties_emu(emulator):
    rs.check_head_ties("cpu")


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rs.LAYER_CASES))
def test_banded_layer(hip_library, name):
    rs.check_layer(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rs.DEC_CASES))
def test_banded_decoder(hip_library, name):
    rs.check_decoder(name, "cuda")


@pytest.mark.gpu
def test_bce(hip_library):
    rs.check_bce("cuda")


@pytest.mark.gpu
def test_ce(hip_library):
    rs.check_ce("cuda")


@pytest.mark.gpu
def test_head_criteria(hip_library):
    rs.check_head_criteria("cuda")


@pytest.mark.gpu
def test_eval_scores(hip_library):
    rs.check_eval_scores("cuda")


@pytest.mark.gpu
def test_masked_loss_edges(hip_library):
    rs.check_masked_loss_edges("cuda")


@pytest.mark.gpu
def test_head_ties(hip_library):
    rs.check_head_ties("cuda")
