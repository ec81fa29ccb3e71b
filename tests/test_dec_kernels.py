"""The persistent decoder kernels (csrc/kernels_decoder.h) at every template instance a decoder reaches, each pinned by one decoder
case against the oracle's decoder in float64 (tests/dec_kernel_suite.py).

Which instance takes a decoder is invisible to every parity test -- all of them compute the same numbers.  The forward has one
instance per hop count (M in {1, 2, 3, 4, 5, 7}); the backward is selected by M, by DT (the weight-group size of its projection
transpose: 5 where Dout / 4 is a multiple of 5, else 4) and by CX0 (column tiles of layer 0's c1 / c2 packs: 12 up to 128 outputs, 16
up to 192, 20 up to 256), within 64 units, 20 nodes, 4 layers, 64 steps and the LDS of a CU.  The suite restates those rules from
the documented geometry.  Without a GPU: the restatement answers as `ops.decoder_is_persistent` (the emulator build of api.cpp)
over the whole grid of shapes, and so does the launch plan (csrc/dec_launch.h through the plan driver), which names the instances the
restatement names; its enumeration gives 6 forward and 32 backward instances, the case table names exactly those, the
shape after each LDS edge is refused, and a share of the table runs on the emulator -- which proves through the event recorder
that the named instances exist and are what a decoder of those dimensions launches.  With a GPU (`-m gpu`): every case proves
through the recorder that the kernels it names took `dec_fwd_persist` and `dec_bwd_persist`, once each, with no per-step decoder
launch beside them; then outputs, dh0 and every parameter gradient against float64, and the forward once more under no_grad
(bit-equal).  Beside the table: 64 steps (the last persistent horizon, with and without flags) and 65 (per-step launches), three
rows at one clip more than the grid (also with a cotangent on three clips only), two rows under dropout."""
import os
import re
import subprocess

import pytest
import torch

import dec_kernel_suite as dk
import quad_gemm_suite as qg
import wide_decoder_suite as wd


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
    torch.set_num_threads(16)             # (the float64 reference: under two seconds for the largest case)
    yield lib


# ---- no GPU: the rules ----------------------------------------------------------------------------------------------------------
GRID = [(t, n, h, dout, m, layers) for m in range(1, 8) for layers in range(1, 6) for dout in range(4, 265, 4) for n in (20, 21)
        for t in (64, 65) for h in (32, 64)]


def test_restated_rules_answer_as_the_library_over_the_whole_grid(emulator):
    from eeg_gnn_ssl_amd import ops
    assert len(GRID) == 7 * 5 * 66 * 2 * 2 * 2
    wrong = [(d, dk.is_persistent(*d)) for d in GRID if ops.decoder_is_persistent(d[0], 2, *d[1:]) is not dk.is_persistent(*d)]
    assert not wrong, "(T, N, H, Dout, M, L), restatement: %s" % wrong[:5]
    accepted = [d for d in GRID if dk.is_persistent(*d)]
    assert len(accepted) >= 32 and {d[:3] for d in accepted} == {(64, 20, 64)}                   # one of the eight (T, N, H) corners holds shapes
    # the capability rows of the wide decoder suite are answered alike; their nodes and steps lie inside the range the grid's corners bound
    for (t, b, n, h, dout, m, layers), want in wd.CAPABILITY:
        assert n <= 20 and t <= 64 and (64, 20, h, dout, m, layers) in GRID
        assert dk.is_persistent(t, n, h, dout, m, layers) is want and ops.decoder_is_persistent(t, b, n, h, dout, m, layers) is want
    # the clip count is no rule, nor are fewer nodes or steps
    for d in ((1, 1, 64, 16, 1, 1), (64, 20, 64, 256, 4, 3), (12, 19, 64, 200, 5, 2)):
        for b in (1, 256, 257, 4096):
            assert ops.decoder_is_persistent(d[0], b, *d[1:]) and dk.is_persistent(*d)


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return qg.build_plan_driver(tmp_path_factory.mktemp("plan_driver"))


def test_launch_plan_answers_as_the_restated_rules_over_the_whole_grid(plan_driver):
    """csrc/dec_launch.h through the plan driver (tests/emu/gemm_plan_driver.cpp, `dec` lines): covered where the restatement says so, as
    the two instances the restatement names, and over the grid exactly the reachable instances"""
    calls = "".join("dec %d 2 %d %d %d %d %d 0 0\n" % d for d in GRID)
    out = subprocess.run([plan_driver], input=calls, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(GRID)
    seen_f, seen_b = set(), set()
    for (t, n, h, dout, m, layers), line in zip(GRID, out):
        fields = line.split(" ; ")
        assert fields[0] == ("1" if dk.is_persistent(t, n, h, dout, m, layers) else "0"), ((t, n, h, dout, m, layers), line)
        if fields[0] == "0":
            assert fields[1:] == ["fwd: per_step", "bwd: per_step"], line
            continue
        assert len(fields) == 5 and fields[2].split()[:3] == fields[4].split()[:3] == ["2", "1", "256"], line
        got = {"dec_fwd_persist": fields[1][len("fwd: "):], "dec_bwd_persist": fields[3][len("bwd: "):]}
        assert got == dk.symbols_of(m, dout), ((m, dout), line)
        assert (int(fields[2].split()[3]), int(fields[4].split()[3])) == (dk.fwd_lds_bytes(m, layers, dout), dk.bwd_lds_bytes(m, layers, dout)), line
        seen_f.add(got["dec_fwd_persist"])
        seen_b.add(got["dec_bwd_persist"])
    assert (seen_f, seen_b) == dk.reachable_instances()


def test_wide_outputs_with_seven_hop_matrices_never_fit_the_lds():
    """no wide backward instance is compiled at M = 7 (dec_has_instance, csrc/dec_launch.h, refuses the pair); the LDS rule alone already
    refuses every such shape, so that rule changes no answer"""
    assert not [d for d in range(132, 257, 4) if dk.fwd_lds_bytes(7, 1, d) <= dk.LDS_BYTES and dk.bwd_lds_bytes(7, 1, d) <= dk.LDS_BYTES]
    assert dk.bwd_lds_bytes(7, 1, 128) == 162944 and dk.fwd_lds_bytes(4, 4, 192) == 162624      # (DESIGN.md 4.4 states the table in bytes)
    assert (dk.fwd_lds_bytes(5, 2, 200), dk.bwd_lds_bytes(5, 2, 200)) == (162112, 152192)


def test_case_table_names_exactly_the_reachable_instances():
    f, b = dk.reachable_instances()
    assert (len(f), len(b)) == (6, 32)
    assert f == {dk.fwd(m) for m in dk.MS}
    assert b == {dk.bwd(m, dt, cx0) for m in dk.MS for dt in (4, 5) for cx0 in (12, 16, 20) if not (m == 7 and cx0 > 12)}
    named_f = {c["expect"]["dec_fwd_persist"] for c in dk.CASES.values()}
    named_b = [c["expect"]["dec_bwd_persist"] for c in dk.CASES.values()]
    assert len(named_b) == len(set(named_b)) == 32, "one row per backward instance"
    assert named_f == f and set(named_b) == b, {"reachable without a case": sorted((f | b) - named_f - set(named_b)),
                                                "named but unreachable": sorted((named_f | set(named_b)) - f - b)}
    for name, c in dk.ALL_CASES.items():
        dims = (c["t"], c["n"], dk.H, c["dout"], c["m"], c["layers"])
        assert c["m"] == dk.hops(c["filt"], c["order"]) == wd.hops(c["filt"], c["order"])
        if c["expect"] is None:
            assert not dk.is_persistent(*dims) and dk.is_persistent(64, *dims[1:]), name        # (the horizon alone refuses it)
            continue
        assert dk.is_persistent(*dims), name
        assert c["expect"] == dk.symbols_of(c["m"], c["dout"]), (name, dk.symbols_of(c["m"], c["dout"]))
        assert re.fullmatch(r"dec_bwd_persist_kernel<64, [123457], [45], (12|16|20)>", c["expect"]["dec_bwd_persist"]), name


def test_lds_edges_and_the_next_shape_out(emulator):
    from eeg_gnn_ssl_amd import ops
    rows = {(c["m"], c["dout"], c["layers"]) for c in dk.CASES.values()}
    for (m, dout, layers), beyond in dk.LDS_EDGES.items():
        assert (m, dout, layers) in rows
        assert dk.is_persistent(64, 20, 64, dout, m, layers) and ops.decoder_is_persistent(64, 2, 20, 64, dout, m, layers)
        assert dk.LDS_BYTES - 2048 < max(dk.fwd_lds_bytes(m, layers, dout), dk.bwd_lds_bytes(m, layers, dout)) <= dk.LDS_BYTES
        for m2, dout2, layers2 in beyond:
            assert dk.dt_of(dout2) != 0 and max(dk.fwd_lds_bytes(m2, layers2, dout2), dk.bwd_lds_bytes(m2, layers2, dout2)) > dk.LDS_BYTES
            assert not dk.is_persistent(1, 1, 64, dout2, m2, layers2) and not ops.decoder_is_persistent(1, 2, 1, 64, dout2, m2, layers2)
    assert dk.is_persistent(64, 20, 64, 80, 5, 4) and ops.decoder_is_persistent(64, 2, 20, 64, 80, 5, 4)
    assert {b for outs in dk.LDS_EDGES.values() for b in outs} == {(4, 208, 4), (5, 160, 3), (5, 220, 2), (5, 224, 2), (7, 140, 1), (7, 80, 2)}


def test_case_table_holds_the_edges_it_is_there_for():
    rows = list(dk.CASES.values())
    douts = {c["dout"] for c in rows}
    assert {80, 160} <= douts and dk.dt_of(80) == dk.dt_of(160) == 5                            # divisible by 4 and by 5
    tiles = {-(-d // 16) for d in douts}
    assert {9, 12, 13, 14, 15, 16} <= tiles and 7 in tiles                                      # wide-tail occupancies; wave 3 without a second tile
    assert {(d // 4) % 4 for d in douts} == {0, 1, 2, 3}                                        # leftover pieces of the quad pack
    for cx0 in (12, 16, 20):
        assert {c["layers"] for c in rows if dk.cx0_of(c["dout"]) == cx0} == {1, 2, 3, 4}
    assert {c["filt"] for c in rows if c["m"] == 4} == {dk.LAP, dk.RW}
    for key, values in (("n", {5, 12, 16, 17, 19, 20}), ("act", {"tanh", "relu"}), ("flags", {None, "host", "device"}), ("sup", {"shared", "per_clip"})):
        assert {c[key] for c in rows} == values, key
        for v in values:
            assert sum(c[key] == v for c in rows) >= 2 and any(c[key] == v and dk.cx0_of(c["dout"]) > 12 for c in rows), (key, v)
    assert all(2 <= c["b"] <= 3 and 2 <= c["t"] <= 4 and not c["dropout"] for c in rows)
    for name, c in dk.ALL_CASES.items():
        mask, seed = dk.flag_mask(c)
        assert (mask is None) == (c["flags"] is None) and (seed is not None) == (c["flags"] == "host"), name
        if mask is not None:                    # mixed outcomes among the steps whose flag matters (the last step feeds nothing)
            assert c["t"] >= 3 and any(mask[:-1]) and not all(mask[:-1]), (name, mask)
        if c["layers"] == 1:                    # one layer (dbias1 aliases dbias0, every pair at l == 0): at least one step feeds back
            assert c["t"] >= 3 and (mask is None or not all(mask[:-1])), name
    assert sum(c["layers"] == 1 for c in rows) >= 6 and any(c["layers"] == 1 and c["flags"] is None for c in rows)
    # the horizon, the walk, dropout
    t64 = dk.T_CASES["t64_flags"]
    assert (t64["m"], t64["dout"], t64["layers"], t64["n"], t64["b"], t64["t"]) == (1, 16, 1, 3, 2, 64) and dk.flag_mask(t64)[0][63]
    assert {c["t"] for c in dk.T65_CASES.values()} == {65} and len(dk.T65_CASES) == 2
    assert {(c["m"], c["dout"], c["layers"], c["b"]) for c in dk.WALK_CASES.values()} == {(4, 96, 2, 257), (5, 208, 2, 257), (1, 256, 4, 257)}
    assert all(c["act"] == "tanh" for c in dk.WALK_CASES.values()) and dk.sparse_clips(257) == [0, 255, 256]
    assert {(c["m"], c["dout"], c["layers"], c["dropout"]) for c in dk.DROPOUT_CASES.values()} == {(4, 100, 3, 0.5), (3, 224, 3, 0.5)}
    # shared supports are 2-D, per-clip ones 3-D and differ between clips
    g = torch.Generator().manual_seed(0)
    for name in ("m2_d112_l2", "m4_d100_l3", "m7_d128_l1", "m4_d96_l2"):
        c = dk.CASES[name]
        sup = dk.make_supports(c, g)
        assert len(sup) == (2 if c["filt"] == dk.DUAL else 1)
        assert all(s.shape == ((c["n"], c["n"]) if c["sup"] == "shared" else (c["b"], c["n"], c["n"])) for s in sup), name
        assert c["sup"] == "shared" or not torch.equal(sup[0][0], sup[0][1]), name


def test_emulator_share_of_the_table():
    emu = [dk.ALL_CASES[name] for name in dk.EMU_CASES]
    table = [dk.CASES[name] for name in dk.EMU_CASES if name in dk.CASES]
    assert {c["m"] for c in table} == set(dk.MS) and {dk.dt_of(c["dout"]) for c in table} == {4, 5}
    assert {dk.cx0_of(c["dout"]) for c in table} == {12, 16, 20} and {1, 4} <= {c["layers"] for c in table}
    assert [name for name, c in dk.CASES.items() if c["m"] == 4] == [name for name in dk.EMU_CASES if name in dk.CASES and dk.CASES[name]["m"] == 4]
    assert "t64_flags" in dk.EMU_CASES and all(c["b"] <= 3 and c["expect"] is not None for c in emu)
    assert {c["expect"]["dec_fwd_persist"] for c in table} == {dk.fwd(m) for m in dk.MS}        # every forward instance launches there


# ---- no GPU: the emulator's share, recorder-proven symbols -------------------------------------------------------------------------
@pytest.mark.parametrize("name", dk.EMU_CASES)
def test_dec_kernel_case_emu(emulator, name):
    dk.check_case(name, "cpu")


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.CASES))
def test_dec_kernel_case(hip_library, name):
    dk.check_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.T_CASES))
def test_dec_kernel_64_steps(hip_library, name):
    dk.check_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.T65_CASES))
def test_dec_kernel_65_steps_take_the_per_step_path(hip_library, name):
    dk.check_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.WALK_CASES))
def test_dec_kernel_walk_case(hip_library, name):
    dk.check_case(name, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.WALK_CASES))
def test_dec_kernel_walk_case_sparse_cotangent(hip_library, name):
    dk.check_case(name, "cuda", sparse=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dk.DROPOUT_CASES))
def test_dec_kernel_dropout_case(hip_library, name):
    dk.check_case(name, "cuda")
