"""EDF recordings decoded on the device, from TUSZ files to clip tables: `eeg_gnn_ssl_amd/edf.py`, `torch.ops.eeg_dcrnn.edf_decode`,
`RecordingDataset.from_edf` (tests/edf_suite.py).  The host checks need no library; every device check runs on the emulator build of
the kernel sources (no GPU) and again, marked `gpu`, on the MI355X library; the index past 2^31 runs on the MI355X only."""
import os

import pytest
import torch

import edf_suite as es

CASES = sorted(es.cases())


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


# ---- no library ----------------------------------------------------------------------------------------------------------------
def test_case_shapes():
    es.check_case_shapes()


def test_parser_reads_what_the_writer_wrote():
    es.check_parser()


def test_parser_refusals():
    es.check_parser_refusals()


def test_select_channels():
    es.check_select_channels()


def test_seizure_times():
    es.check_seizure_times()


def test_marker_lists_to_clip_tables():
    es.check_markers()


def test_committed_file_on_the_host():
    es.check_golden_host()


def test_fake_implementation():
    es.check_fake()


# ---- emulator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cases_emu(emulator, name):
    es.check_case("cpu", name)


def test_one_record_slices_emu(emulator):
    es.check_one_record_slices("cpu")


def test_guarded_output_emu(emulator):
    es.check_guarded_output("cpu")


def test_invariance_emu(emulator):
    es.check_invariance("cpu")


def test_committed_file_emu(emulator):
    es.check_golden_device("cpu")


def test_refusals_emu(emulator):
    es.check_refusals("cpu")


def test_end_to_end_emu(emulator):
    es.check_end_to_end("cpu")


def test_pyedflib_emu(emulator):
    es.check_pyedflib("cpu")


# ---- MI355X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_cases(hip_library, name):
    es.check_case("cuda", name)


@pytest.mark.gpu
def test_one_record_slices(hip_library):
    es.check_one_record_slices("cuda")


@pytest.mark.gpu
def test_guarded_output(hip_library):
    es.check_guarded_output("cuda")


@pytest.mark.gpu
def test_invariance(hip_library):
    es.check_invariance("cuda")


@pytest.mark.gpu
def test_committed_file(hip_library):
    es.check_golden_device("cuda")


@pytest.mark.gpu
def test_large_index(hip_library):
    es.check_large_index("cuda")


@pytest.mark.gpu
def test_refusals(hip_library):
    es.check_refusals("cuda")


@pytest.mark.gpu
def test_end_to_end(hip_library):
    es.check_end_to_end("cuda")


@pytest.mark.gpu
def test_pyedflib(hip_library):
    es.check_pyedflib("cuda")
