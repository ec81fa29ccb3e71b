"""Checks of the EDF front end (eeg_gnn_ssl_amd/edf.py, `torch.ops.eeg_dcrnn.edf_decode`, `RecordingDataset.from_edf`), run by
tests/test_edf.py on the emulator build ("cpu") and on the MI355X library ("cuda").

Yardstick: `restate`, a float64 numpy restatement of the decode written from the EDF specification and EDFlib's formula
    physical = gain * (offset + digital),  gain = (pmax - pmin) / (dmax - dmin),  offset = pmax / gain - dmax
over the int16 of the payload at index r * R + chan_off + j.  It reads the signal table the WRITER (`write_edf`) was given, not the
parser's header, so parser, writer and kernel are checked against each other; tests/golden/tiny_v1.edf + tiny_v1.npz (written once by
`python tests/edf_suite.py --write-golden`) keep a later change to writer and parser together from passing unnoticed.

Tolerance: none.  Each output element is one correctly rounded float64 add and one correctly rounded float64 multiply of the same
operands: float64 results are `torch.equal` to the restatement, float32 results to its `.astype(float32)` (one more rounding).

TILE restates kEdfTile of csrc/kernels_edf.h: a workgroup writes TILE consecutive samples of one output row.  Inputs are closed forms:
no draws."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
TINY_EDF = os.path.join(GOLDEN_DIR, "tiny_v1.edf")
TINY_NPZ = os.path.join(GOLDEN_DIR, "tiny_v1.npz")
TINY_TSE = os.path.join(GOLDEN_DIR, "tiny_v1.tse_bi")
MARKERS = os.path.join(GOLDEN_DIR, "markers_v1")
TILE = 1024
MAX_CHANNELS = 32
PMIN, PMAX = -5482.28, 5482.288                                          # TUSZ-like physical range over -32767 .. 32767, as 8 header characters hold it
CHANNELS = ["EEG FP1", "EEG FP2", "EEG F3", "EEG F4", "EEG C3", "EEG C4", "EEG P3", "EEG P4", "EEG O1", "EEG O2", "EEG F7", "EEG F8", "EEG T3",
            "EEG T4", "EEG T5", "EEG T6", "EEG FZ", "EEG CZ", "EEG PZ"]


# ---- the writer and the restatement (independent of eeg_gnn_ssl_amd/edf.py) -------------------------------------------------------
def sig(label, nsamp, pmin=PMIN, pmax=PMAX, dmin=-32767, dmax=32767):
    return dict(label=label, nsamp=nsamp, pmin=pmin, pmax=pmax, dmin=dmin, dmax=dmax, transducer="AgAgCl electrode", dimension="uV",
                prefilter="HP:0.1Hz LP:75Hz")


def digital(s, length, extremes=False):
    """the int16 samples of signal s: a closed form that fills the whole range; `extremes` plants -32768, -1, 0, 32767"""
    t = np.arange(length, dtype=np.int64)
    d = ((t * 7919 + s * 10007 + (t * t) % 8191 * 13 + (t // 5) * 331) % 65536 - 32768).astype(np.int16)
    if extremes:
        d[:4] = [-32768, -1, 0, 32767]
        d[-4:] = [32767, 0, -1, -32768]
    return d


def _field(value, width):
    text = value if isinstance(value, str) else repr(value) if isinstance(value, float) else str(value)
    if isinstance(value, float) and text.endswith(".0"):
        text = text[:-2]
    assert len(text) <= width, (text, width)
    return text.ljust(width).encode("ascii")


def write_edf(signals, num_records, data=None, record_duration=1.0, reserved="", version="0", declared_records=None, header_bytes=None,
              patient="X X X X", recording="Startdate X X X X", start_date="01.01.01", start_time="00.00.00", extremes=False):
    """an EDF file as bytes: the 256-byte fixed block, the field-major signal blocks, then num_records records of each signal's nsamp
    little-endian int16 in file order.  data[s]: int16 (num_records * nsamp[s]), default `digital`."""
    ns = len(signals)
    if data is None:
        data = [digital(s, num_records * g["nsamp"], extremes) for s, g in enumerate(signals)]
    head = [_field(version, 8), _field(patient, 80), _field(recording, 80), _field(start_date, 8), _field(start_time, 8),
            _field(256 * (ns + 1) if header_bytes is None else header_bytes, 8), _field(reserved, 44),
            _field(num_records if declared_records is None else declared_records, 8), _field(record_duration, 8), _field(ns, 4)]
    for key, width in (("label", 16), ("transducer", 80), ("dimension", 8), ("pmin", 8), ("pmax", 8), ("dmin", 8), ("dmax", 8), ("prefilter", 80),
                       ("nsamp", 8), (None, 32)):
        head += [_field("" if key is None else g[key], width) for g in signals]
    head = b"".join(head)
    assert len(head) == 256 * (ns + 1)
    records = []
    for r in range(num_records):
        for s, g in enumerate(signals):
            d = np.asarray(data[s])
            assert d.dtype == np.int16 and d.shape == (num_records * g["nsamp"],)
            records.append(d[r * g["nsamp"]:(r + 1) * g["nsamp"]].astype("<i2").tobytes())
    return head + b"".join(records)


def scaling(g):
    """(gain, offset) of a signal of the writer's table, float64"""
    gain = (np.float64(g["pmax"]) - np.float64(g["pmin"])) / (np.float64(g["dmax"]) - np.float64(g["dmin"]))
    return float(gain), float(np.float64(g["pmax"]) / gain - np.float64(g["dmax"]))


def layout(signals, picked):
    """(R, n, chan_off, gain, offset) of the picked signals of a writer's table"""
    nsamp = [g["nsamp"] for g in signals]
    n = nsamp[picked[0]]
    assert all(nsamp[s] == n for s in picked)
    sc = [scaling(signals[s]) for s in picked]
    return sum(nsamp), n, [sum(nsamp[:s]) for s in picked], [a for a, _ in sc], [b for _, b in sc]


def restate(payload, num_records, R, n, chan_off, gain, offset):
    """payload bytes -> (C, num_records * n) float64: gain * (offset + int16 at r * R + chan_off + j), one add, one multiply"""
    d = np.frombuffer(bytes(payload), dtype="<i2", count=num_records * R).reshape(num_records, R)
    out = np.empty((len(chan_off), num_records * n), dtype=np.float64)
    for c, (off, g, o) in enumerate(zip(chan_off, gain, offset)):
        out[c] = np.float64(g) * (np.float64(o) + d[:, off:off + n].reshape(-1).astype(np.float64))
    return out


# ---- the decode cases of the issue -------------------------------------------------------------------------------------------------
def _tusz33():
    """33 signals in an order that is not the montage's: the 19 channels reversed, unselected signals of other rates between them, a
    57-sample annotation signal in front and a SECOND 'EEG FP1' behind the first (the first match wins)"""
    table = [sig("EDF Annotations", 57, -1, 1, -32768, 32767)]
    extras = [sig("EEG A1-REF", 256), sig("EEG EKG1-REF", 256), sig("PHOTIC-REF", 1, -1, 1, -32768, 32767), sig("IBI", 1, 0, 100, 0, 32767),
              sig("BURSTS", 3, -8, 8, -32767, 32767), sig("SUPPR", 5), sig("EEG A2-REF", 256), sig("EEG T1-REF", 128), sig("EEG T2-REF", 128),
              sig("EEG ROC-REF", 256), sig("EEG LOC-REF", 256), sig("EMG-REF", 512), sig("EEG FP1-REF", 256, -100.0, 100.0, -2048, 2047)]
    for k, name in enumerate(reversed(CHANNELS)):
        table.append(sig(name + "-REF", 256, round(PMIN - k, 3), round(PMAX + 2 * k, 3)))
        if k < len(extras):
            table.append(extras[k])
    assert len(table) == 33
    return table


def _case(signals, num_records, picked=None, extremes=False):
    return dict(signals=signals, num_records=num_records, picked=list(range(len(signals))) if picked is None else picked, extremes=extremes)


def _pick_by_name(table, names):
    labels = [g["label"].split("-")[0] for g in table]
    return [labels.index(name) for name in names]


def cases():
    t33 = _tusz33()
    return {
        "plain": _case([sig(name + "-REF", 250) for name in CHANNELS], 2),
        "odd_R": _case([sig("EDF Annotations", 57, -1, 1, -32768, 32767)] + [sig(name + "-LE", 250) for name in CHANNELS], 3, list(range(1, 20))),
        "n1": _case([sig("PAD", 2), sig("A", 1), sig("B", 1), sig("C", 1)], 5, [1, 2, 3]),
        "n3": _case([sig("PAD", 2), sig("A", 3), sig("B", 3), sig("PAD2", 1), sig("C", 3)], 5, [4, 1, 2]),
        "tusz33": _case(t33, 2, _pick_by_name(t33, CHANNELS)),
        "one_record": _case([sig("PAD", 3), sig("A", 250), sig("B", 250)], 1, [2, 1]),
        "n256_r7": _case([sig("A", 256), sig("PAD", 1), sig("B", 256)], 7, [0, 2]),
        "n1000_r7": _case([sig("PAD", 1), sig("A", 1000), sig("B", 1000)], 7, [1, 2]),
        "extremes": _case([sig("A", 16), sig("INV", 16, PMAX, PMIN), sig("B", 16, -3276.8, 3276.7, -32768, 32767), sig("C", 16, -100.0, 101.5, -2048, 2047)],
                          3, [0, 1, 2, 3], extremes=True),
    }


def build(case):
    """-> (file bytes, payload bytes, num_records, R, n, chan_off, gain, offset, float64 reference)"""
    file = write_edf(case["signals"], case["num_records"], extremes=case["extremes"])
    payload = file[256 * (len(case["signals"]) + 1):]
    R, n, chan_off, gain, offset = layout(case["signals"], case["picked"])
    assert len(payload) == 2 * case["num_records"] * R
    return file, payload, case["num_records"], R, n, chan_off, gain, offset, restate(payload, case["num_records"], R, n, chan_off, gain, offset)


def _bytes_tensor(b, device):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to(device)


def _nan(*shape, device, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _want(ref, dtype):
    return torch.from_numpy(ref if dtype == torch.float64 else ref.astype(np.float32))


# ---- no GPU, no library ------------------------------------------------------------------------------------------------------------
def check_case_shapes():
    """the cases are what the issue says: parities, tiles, extreme values, a non-integer offset"""
    cs = cases()
    R, n, off, _, _ = layout(cs["plain"]["signals"], cs["plain"]["picked"])
    assert (R, n, len(off), cs["plain"]["num_records"]) == (19 * 250, 250, 19, 2)
    R, n, off, _, _ = layout(cs["odd_R"]["signals"], cs["odd_R"]["picked"])
    assert R % 2 == 1 and all(o % 2 == 1 for o in off) and cs["odd_R"]["num_records"] == 3
    assert {(r * R + off[0]) % 2 for r in range(3)} == {0, 1}, "a channel's runs must begin on both 4-byte parities"
    assert layout(cs["n1"]["signals"], cs["n1"]["picked"])[1] == 1 and layout(cs["n3"]["signals"], cs["n3"]["picked"])[1] == 3
    t = cs["tusz33"]
    assert len(t["signals"]) == 33 and len(t["picked"]) == 19 and t["picked"] != sorted(t["picked"])
    labels = [g["label"].split("-")[0] for g in t["signals"]]
    assert labels.count("EEG FP1") == 2 and t["picked"][0] == labels.index("EEG FP1")
    between = {g["nsamp"] for g in t["signals"][min(t["picked"]):max(t["picked"])]}
    assert between - {256}, "unselected signals of other nsamp must lie between the selected ones"
    R, n, off, _, _ = layout(cs["one_record"]["signals"], cs["one_record"]["picked"])
    assert cs["one_record"]["num_records"] == 1 and max(off) + n == R, "the last run must end on the last payload byte"
    for name in ("n256_r7", "n1000_r7"):
        R, n, off, _, _ = layout(cs[name]["signals"], cs[name]["picked"])
        L = cs[name]["num_records"] * n
        assert L % TILE != 0 and L > TILE, (name, L)
        assert any((r * n) % TILE != 0 for r in range(1, cs[name]["num_records"])), f"{name}: no record boundary inside a tile"
    assert any((k * TILE) % 1000 != 0 for k in range(1, 7000 // TILE + 1)), "n = 1000: no tile boundary inside a record"
    e = cs["extremes"]
    data = [digital(s, 3 * 16, True) for s in range(4)]
    assert all({-32768, -1, 0, 32767} <= set(d.tolist()) for d in data)
    gains = [scaling(g) for g in e["signals"]]
    assert gains[1][0] < 0 < gains[0][0], "one channel has inverted polarity"
    assert gains[0][1] != round(gains[0][1]) and gains[3][1] != round(gains[3][1]), "the offsets must not be integers"


def check_parser():
    """read_edf_header against the writer, every field, for every case; -1 records; EDF+C accepted"""
    from eeg_gnn_ssl_amd import read_edf_header
    for name, case in cases().items():
        file = write_edf(case["signals"], case["num_records"], record_duration=0.5 if name == "n3" else 1.0, patient="P " + name,
                         recording="Startdate 02-MAR-2002 " + name, start_date="02.03.02", start_time="11.22.33")
        for source in (file, np.frombuffer(file, dtype=np.uint8)):
            h = read_edf_header(source)
            sigs = case["signals"]
            assert h.version == "0" and h.patient == "P " + name and h.recording == "Startdate 02-MAR-2002 " + name
            assert h.start_date == "02.03.02" and h.start_time == "11.22.33" and h.reserved == ""
            assert h.header_bytes == 256 * (len(sigs) + 1) and h.ns == len(sigs) and h.num_records == case["num_records"]
            assert h.record_duration == (0.5 if name == "n3" else 1.0)
            assert h.labels == [g["label"] for g in sigs] and h.nsamp == [g["nsamp"] for g in sigs]
            assert h.pmin == [float(g["pmin"]) for g in sigs] and h.pmax == [float(g["pmax"]) for g in sigs]
            assert h.dmin == [g["dmin"] for g in sigs] and h.dmax == [g["dmax"] for g in sigs]
            assert h.transducers == [g["transducer"] for g in sigs] and h.dimensions == [g["dimension"] for g in sigs]
            assert h.prefilters == [g["prefilter"] for g in sigs]
            assert h.record_len == sum(g["nsamp"] for g in sigs) and h.payload_bytes == len(file) - h.header_bytes
            for s, g in enumerate(sigs):
                assert h.chan_off(s) == sum(x["nsamp"] for x in sigs[:s]) and h.gain_offset(s) == scaling(g), (name, s)
    table = [sig("A", 5), sig("B", 3)]
    file = write_edf(table, 4, declared_records=-1)
    assert read_edf_header(file).num_records == 4
    assert read_edf_header(file + b"\x00" * 15).num_records == 4 and read_edf_header(file[:-1]).num_records == 3      # whole records only
    assert read_edf_header(write_edf(table, 2, reserved="EDF+C")).reserved == "EDF+C"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "a.edf")
        with open(path, "wb") as f:
            f.write(file)
        assert read_edf_header(path).num_records == 4 and read_edf_header(path).labels == ["A", "B"]


def check_parser_refusals():
    """every refusal of read_edf_header is a ValueError that names the field"""
    from eeg_gnn_ssl_amd import read_edf_header
    table = [sig("A", 5), sig("B", 3)]
    bad = lambda key, value: [dict(table[0], **{key: value}), table[1]]      # noqa: E731
    good = write_edf(table, 2)
    ns_at = 252
    for file, text in (
            (write_edf(table, 2, version="1"), r"version='1'"),
            (b"\xffBIOSEMI" + good[8:], r"version=.*BIOSEMI.*BDF"),
            (write_edf(table, 2, reserved="EDF+D"), r"reserved='EDF\+D'"),
            (write_edf(table, 2, header_bytes=512), r"header_bytes=512 for ns=2"),
            (good[:ns_at] + b"0   " + good[ns_at + 4:], r"ns=0"),
            (good[:ns_at] + b"-1  " + good[ns_at + 4:], r"ns=-1"),
            (good[:ns_at] + b"two " + good[ns_at + 4:], r"ns='two' is not a number"),
            (write_edf(table, 2, header_bytes="abc"), r"header_bytes='abc' is not a number"),
            (write_edf(table, 2, declared_records="x"), r"num_records='x' is not a number"),
            (write_edf(table, 2, record_duration="1s"), r"record_duration='1s' is not a number"),
            (write_edf(bad("pmin", "lo"), 2), r"physical_min\[0\]='lo' is not a number"),
            (write_edf(bad("pmax", "hi"), 2), r"physical_max\[0\]='hi' is not a number"),
            (write_edf(bad("dmin", "1.5"), 2), r"digital_min\[0\]='1.5' is not a number"),
            (write_edf(bad("dmax", ""), 2), r"digital_max\[0\]='' is not a number"),
            (write_edf(table, 2, record_duration=0), r"record_duration='0' must be a positive"),
            (write_edf(table, 2, record_duration=-1.0), r"record_duration='-1' must be a positive"),
            (write_edf(table, 2, declared_records=3), r"num_records=3 records of 16 bytes need 48 payload bytes, the file has 32"),
            (good[:-1], r"num_records=2 .* the file has 31"),
            (write_edf(table, 2, declared_records=-2), r"num_records=-2"),
            (good[:100], r"header_bytes: the file has 100 bytes"),
            (good[:600], r"header_bytes=768, the file has 600 bytes"),
    ):
        with pytest.raises(ValueError, match=text):
            read_edf_header(file)
    # (the writer refuses to slice nsamp = 0 data, so these two headers are patched into a good file)
    at = 256 + 2 * (16 + 80 + 8 + 8 + 8 + 8 + 8 + 80)
    with pytest.raises(ValueError, match=r"samples_per_record\[0\]=0"):
        read_edf_header(good[:at] + b"0       " + good[at + 8:])
    with pytest.raises(ValueError, match=r"samples_per_record\[1\]='n' is not a number"):
        read_edf_header(good[:at + 8] + b"n       " + good[at + 16:])
    with pytest.raises(ValueError, match=r"digital_max\[0\] == digital_min\[0\] == 7"):
        read_edf_header(write_edf([dict(table[0], dmin=7, dmax=7), table[1]], 2))
    with pytest.raises(ValueError, match=r"source must be a path, bytes or a 1-D uint8 array"):
        read_edf_header(np.zeros(4, dtype=np.int16))


def check_select_channels():
    """the reference's rule on -REF and -LE labels: cut at the first '-', the first match wins; the two refusals; the rate"""
    from eeg_gnn_ssl_amd import read_edf_header, select_channels
    for suffix in ("-REF", "-LE"):
        table = [sig("EDF Annotations", 57)] + [sig(name + suffix, 250) for name in reversed(CHANNELS)] + [sig("EEG FP1" + suffix, 250), sig("EEG A1" + suffix, 250)]
        h = read_edf_header(write_edf(table, 1))
        assert select_channels(h) == [19 - k for k in range(19)], suffix
        assert select_channels(h, ["EEG A1", "EEG FP1"]) == [21, 19]
    cut = [sig("EEG T3-T5-REF", 10), sig("EEG T3", 10)]                   # 'EEG T3-T5-REF' -> 'EEG T3': the first '-' cuts
    assert select_channels(read_edf_header(write_edf(cut, 1)), ["EEG T3"]) == [0]
    h = read_edf_header(write_edf([sig(name + "-REF", 250) for name in CHANNELS[:-1]], 1))
    with pytest.raises(ValueError, match=r"channel 'EEG PZ' is not among"):
        select_channels(h)
    h = read_edf_header(write_edf([sig("A-REF", 250), sig("B-REF", 256)], 1))
    with pytest.raises(ValueError, match=r"channel 'B' has samples_per_record=256, channel 'A' has 250"):
        select_channels(h, ["A", "B"])
    with pytest.raises(ValueError, match=r"no channels"):
        select_channels(h, [])


def check_seizure_times():
    from eeg_gnn_ssl_amd import read_seizure_times
    want = [[10.5, 42.25], [100.0, 163.7812], [300.0, 301.0]]
    assert read_seizure_times(TINY_TSE) == want
    assert read_seizure_times(TINY_EDF) == want                           # the .tse_bi beside the .edf


def check_markers():
    """the three marker readers and recording_ids on 10-line excerpts of the reference's lists; the tables they produce through
    clip_table_* against hand-computed rows"""
    from eeg_gnn_ssl_amd import (clip_table_classification, clip_table_detection, clip_table_ssl, read_markers_classification, read_markers_detection,
                                 read_markers_ssl, recording_ids)
    # detection: NAME.edf_K.h5,label
    names, idx, labels = read_markers_detection(os.path.join(MARKERS, "detection_balanced_trainSet_seq2seq_12s.txt"))
    assert names == ["00010480_s013_t013.edf", "00003636_s001_t001.edf", "00011580_s001_t019.edf", "00011580_s005_t006.edf", "00010587_s001_t000.edf",
                     "00009370_s004_t001.edf", "00010461_s001_t000.edf", "00008616_s001_t000.edf", "00010421_s001_t000.edf", "00011333_s012_t001.edf"]
    assert idx.dtype == np.int64 and idx.tolist() == [19, 2, 64, 23, 1, 41, 40, 148, 33, 40]
    assert labels.dtype == np.int64 and labels.tolist() == [0, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    paths = [os.path.join("/data/tusz/train", n[:3], n) for n in sorted(names)] + ["/data/tusz/dev/other/00000001_s001_t000.edf"]
    ids = recording_ids(names, paths)
    assert ids.dtype == np.int64 and ids.tolist() == [5, 0, 8, 9, 6, 2, 4, 1, 3, 7]
    table = clip_table_detection(ids, idx, 12)
    assert np.asarray(table).tolist() == [[5, 45600, 2400, 0], [0, 4800, 2400, 0], [8, 153600, 2400, 0], [9, 55200, 2400, 0], [6, 2400, 2400, 0],
                                          [2, 98400, 2400, 0], [4, 96000, 2400, 0], [1, 355200, 2400, 0], [3, 79200, 2400, 0], [7, 96000, 2400, 0]]
    # ssl: NAME.edf_Kx.h5,NAME.edf_Ky.h5
    names, kx, ky = read_markers_ssl(os.path.join(MARKERS, "ssl_devSet_seq2seq_12s.txt"))
    assert names == ["00012484_s003_t007.edf"] * 10 and kx.tolist() == list(range(10)) and ky.tolist() == list(range(1, 11))
    ids = recording_ids(names, ["a/b/00000001_s001_t000.edf", "a/c/00012484_s003_t007.edf"])
    assert ids.tolist() == [1] * 10
    table = clip_table_ssl(ids, kx, ky, 12)
    assert np.asarray(table).tolist() == [[1, 2400 * k, 2400, 2400 * (k + 1)] for k in range(10)]
    # classification: NAME.edf,class,seizure_idx
    names, classes, sidx = read_markers_classification(os.path.join(MARKERS, "classification_devSet_seizure_files.txt"))
    assert names == ["00006514_s019_t001.edf", "00004456_s015_t002.edf", "00004456_s015_t002.edf", "00006514_s019_t001.edf", "00006175_s003_t006.edf",
                     "00008476_s001_t000.edf", "00006514_s012_t002.edf", "00004456_s015_t006.edf", "00006175_s002_t000.edf", "00001006_s001_t001.edf"]
    assert classes.tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 0, 1] and sidx.tolist() == [17, 4, 1, 9, 3, 5, 0, 0, 8, 0]
    uniq = sorted(set(names))
    ids = recording_ids(names, uniq)
    assert len(uniq) == 8 and ids.tolist() == [6, 1, 1, 6, 4, 7, 5, 2, 3, 0]
    # hand-written annotations.  Even recordings: seizure k runs 30 k + 10 .. 30 k + 17.5 s (a short seizure: the clip starts 2 s before
    # it, at 200 * (30 k + 8), and ends with it, 1900 samples); odd recordings: 20 k + 10 .. 20 k + 29 s (the seizure before ends 1 s
    # before: the clip starts one sample behind it, at 200 * (20 k + 9) + 1, and is cut at 12 s; seizure 0 starts at 200 * 8)
    even = [[30.0 * k + 10.0, 30.0 * k + 17.5] for k in range(20)]
    odd = [[20.0 * k + 10.0, 20.0 * k + 29.0] for k in range(20)]
    table = clip_table_classification(ids, [odd if r % 2 else even for r in ids.tolist()], sidx, 12)
    assert np.asarray(table).tolist() == [[6, 103600, 1900, 0], [1, 17801, 2400, 0], [1, 5801, 2400, 0], [6, 55600, 1900, 0], [4, 19600, 1900, 0],
                                          [7, 21801, 2400, 0], [5, 1600, 2400, 0], [2, 1600, 1900, 0], [3, 33801, 2400, 0], [0, 1600, 1900, 0]]
    # refusals
    for fn, text in ((lambda: recording_ids(["x.edf"], uniq), r"recording 'x.edf' is not among the 8 edf_paths"),
                     (lambda: recording_ids(names, ["a/" + uniq[0], "b/" + uniq[0]]), r"share the basename")):
        with pytest.raises(ValueError, match=text):
            fn()
    with tempfile.TemporaryDirectory() as tmp:
        for reader, line, text in ((read_markers_detection, "a.edf_1.h5", r"1 comma-separated fields, 2 expected"),
                                   (read_markers_detection, "a.edf_x.h5,1", r"'a.edf_x.h5' is not NAME.edf_K.h5"),
                                   (read_markers_detection, "a.edf_1.h5,yes", r"'yes' is not an integer"),
                                   (read_markers_ssl, "a.edf_1.h5,b.edf_2.h5", r"the input is a clip of 'a.edf', the target of 'b.edf'"),
                                   (read_markers_classification, "a.h5,1,2", r"'a.h5' is not NAME.edf"),
                                   (read_markers_classification, "a.edf,1", r"2 comma-separated fields, 3 expected")):
            path = os.path.join(tmp, "m.txt")
            with open(path, "w") as f:
                f.write(line + "\n")
            with pytest.raises(ValueError, match=text):
                reader(path)


def _tiny():
    table = [sig("EDF Annotations", 3, -1, 1, -32768, 32767), sig("EEG FP1-REF", 8), sig("EEG FP2-REF", 8, PMAX, PMIN), sig("EEG F3-LE", 8, -3276.8, 3276.7, -32768, 32767)]
    return table, 5


def tiny_bytes():
    table, records = _tiny()
    return write_edf(table, records, record_duration=0.04, extremes=True, patient="tiny v1", recording="Startdate 01-JAN-2001 tiny")


def write_golden():
    table, records = _tiny()
    file = tiny_bytes()
    with open(TINY_EDF, "wb") as f:
        f.write(file)
    R, n, off, gain, offset = layout(table, [1, 2, 3])
    np.savez(TINY_NPZ, physical=restate(file[256 * 5:], records, R, n, off, gain, offset), digital=np.stack([digital(s, records * 8, True) for s in (1, 2, 3)]),
             nsamp=np.array([g["nsamp"] for g in table]), pmin=np.array([g["pmin"] for g in table], dtype=np.float64),
             pmax=np.array([g["pmax"] for g in table], dtype=np.float64), dmin=np.array([g["dmin"] for g in table]), dmax=np.array([g["dmax"] for g in table]),
             labels=np.array([g["label"] for g in table]), gain=np.array(gain), offset=np.array(offset), chan_off=np.array(off),
             num_records=records, record_duration=0.04, sample_freq=8 / 0.04)
    with open(TINY_TSE, "w") as f:
        f.write("version = tse_v1.0.0\n\n0.0000 10.5000 bckg 1.0000\n10.5000 42.2500 seiz 1.0000\n42.2500 100.0000 bckg 1.0000\n"
                "100.0000 163.7812 seiz 1.0000\n163.7812 300.0000 bckg 1.0000\n300.0000 301.0000 seiz 1.0000\n301.0000 400.0000 bckg 1.0000\n")


def check_golden_host():
    """the committed file: the writer still produces its bytes, the parser still reads its fields, the restatement its arrays"""
    from eeg_gnn_ssl_amd import read_edf_header, select_channels
    with open(TINY_EDF, "rb") as f:
        file = f.read()
    assert file == tiny_bytes(), "the writer no longer produces the committed fixture"
    h = read_edf_header(TINY_EDF)
    with np.load(TINY_NPZ) as z:
        assert h.labels == z["labels"].tolist() and h.nsamp == z["nsamp"].tolist() and h.num_records == int(z["num_records"])
        assert h.pmin == z["pmin"].tolist() and h.pmax == z["pmax"].tolist() and h.dmin == z["dmin"].tolist() and h.dmax == z["dmax"].tolist()
        assert h.record_duration == float(z["record_duration"]) and h.header_bytes == 1280 and h.record_len == 27
        assert h.patient == "tiny v1" and h.recording == "Startdate 01-JAN-2001 tiny"
        picked = select_channels(h, ["EEG FP1", "EEG FP2", "EEG F3"])
        assert picked == [1, 2, 3] and [h.chan_off(s) for s in picked] == z["chan_off"].tolist()
        assert [h.gain_offset(s)[0] for s in picked] == z["gain"].tolist() and [h.gain_offset(s)[1] for s in picked] == z["offset"].tolist()
        got = restate(file[h.header_bytes:], h.num_records, h.record_len, 8, z["chan_off"].tolist(), z["gain"].tolist(), z["offset"].tolist())
        assert np.array_equal(got, z["physical"])
        want = z["gain"][:, None] * (z["offset"][:, None] + z["digital"].astype(np.float64))
        assert np.array_equal(want, z["physical"])


def check_fake():
    """the operator under FakeTensorMode: shape and dtype, no data"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eeg_gnn_ssl_amd  # noqa: F401
    with FakeTensorMode():
        p = torch.empty(2 * 7 * 40, dtype=torch.uint8)
        for dtype in (torch.float64, torch.float32):
            y = torch.ops.eeg_dcrnn.edf_decode(p, 7, 40, 9, [0, 9, 31], [1.0, 2.0, 3.0], [0.0, 0.5, -1.0], dtype)
            assert tuple(y.shape) == (3, 63) and y.dtype == dtype
        y = torch.ops.eeg_dcrnn.edf_decode(p, 7, 40, 9, [0], [1.0], [0.0])
        assert tuple(y.shape) == (1, 63) and y.dtype == torch.float64
    y = torch.ops.eeg_dcrnn.edf_decode(torch.empty(560, dtype=torch.uint8, device="meta"), 7, 40, 9, [0, 9], [1.0, 2.0], [0.0, 0.5], torch.float32)
    assert y.device.type == "meta" and tuple(y.shape) == (2, 63) and y.dtype == torch.float32


# ---- the operator -------------------------------------------------------------------------------------------------------------------
def check_case(device, name):
    """one decode case, both output types: the operator on the suite's own layout, and `decode_edf` (parser + channel pick + upload +
    operator) on the file"""
    from eeg_gnn_ssl_amd import decode_edf
    case = cases()[name]
    file, payload, records, R, n, off, gain, offset, ref = build(case)
    p = _bytes_tensor(payload, device)
    names = [case["signals"][s]["label"].split("-")[0] for s in case["picked"]]
    for dtype in (torch.float64, torch.float32):
        y = torch.ops.eeg_dcrnn.edf_decode(p, records, R, n, off, gain, offset, dtype)
        assert tuple(y.shape) == (len(off), records * n) and y.dtype == dtype and y.is_contiguous()
        assert torch.equal(y.cpu(), _want(ref, dtype)), f"case {name} {dtype}: the operator differs from the restatement"
        z, fs, header = decode_edf(file, names, dtype=dtype, device=device)
        assert fs == float(n) and header.num_records == records and header.record_len == R
        assert torch.equal(z.cpu(), _want(ref, dtype)), f"case {name} {dtype}: decode_edf differs from the restatement"


def check_one_record_slices(device):
    """one record whose last run ends on the last payload byte, as a slice of a larger byte buffer at 4-byte and at 2-byte alignment,
    with two different fills around it: identical results"""
    case = cases()["one_record"]
    _, payload, records, R, n, off, gain, offset, ref = build(case)
    host = np.frombuffer(payload, dtype=np.uint8)
    for dtype in (torch.float64, torch.float32):
        got = []
        for lead in (0, 2, 4, 6):
            for fill in (0x00, 0xFF, 0x7F):
                big = torch.full((lead + len(host) + 64,), fill, dtype=torch.uint8, device=device)
                big[lead:lead + len(host)] = torch.from_numpy(host.copy()).to(device)
                p = big[lead:lead + len(host)]
                assert p.data_ptr() % 2 == 0 and (lead % 4 == 0 or p.data_ptr() % 4 == 2)
                got.append(torch.ops.eeg_dcrnn.edf_decode(p, records, R, n, off, gain, offset, dtype))
        for g in got:
            assert torch.equal(g.cpu(), _want(ref, dtype)), "the bytes around the payload changed the result"


def check_guarded_output(device):
    """`edf_decode_into` rows inside a larger NaN-filled buffer with out_stride > L: the padding behind each row and the guards on both
    sides keep their bits"""
    from eeg_gnn_ssl_amd import ops
    for name in ("odd_R", "n1000_r7", "n1"):
        _, payload, records, R, n, off, gain, offset, ref = build(cases()[name])
        p = _bytes_tensor(payload, device)
        C, L = len(off), records * n
        for dtype in (torch.float64, torch.float32):
            stride, guard = L + 5, 37
            flat = _nan(guard + C * stride + guard, device=device, dtype=dtype)
            flat.view(torch.int64 if dtype == torch.float64 else torch.int32)[::3] += 12345          # a NaN PATTERN, not one value
            before = flat.clone()
            out = flat[guard:guard + C * stride].view(C, stride)[:, :L]
            assert ops.edf_decode_into(p, records, R, n, off, gain, offset, out) is out
            assert torch.equal(out.cpu(), _want(ref, dtype)), (name, dtype)
            keep = torch.ones(flat.shape, dtype=torch.bool, device=device)
            keep[guard:guard + C * stride].view(C, stride)[:, :L] = False
            assert torch.equal(_bits(flat)[keep], _bits(before)[keep]), f"{name} {dtype}: something outside the output rows was written"


def check_invariance(device):
    """a channel subset equals the same rows of the full decode (any order, repeats allowed); a repeat into a poisoned out gives the
    same bits"""
    from eeg_gnn_ssl_amd import ops
    case = cases()["tusz33"]
    _, payload, records, R, n, off, gain, offset, ref = build(case)
    p = _bytes_tensor(payload, device)
    for dtype in (torch.float64, torch.float32):
        full = torch.ops.eeg_dcrnn.edf_decode(p, records, R, n, off, gain, offset, dtype)
        for rows in ([0], [18, 3, 3, 7], list(range(0, 19, 2))):
            pick = lambda v: [v[r] for r in rows]                             # noqa: E731
            part = torch.ops.eeg_dcrnn.edf_decode(p, records, R, n, pick(off), pick(gain), pick(offset), dtype)
            assert torch.equal(_bits(part), _bits(full[rows])), (dtype, rows)
        out = _nan(len(off), records * n, device=device, dtype=dtype)
        ops.edf_decode_into(p, records, R, n, off, gain, offset, out)
        assert torch.equal(_bits(out), _bits(full))
        out.fill_(-7.0)
        ops.edf_decode_into(p, records, R, n, off, gain, offset, out)
        assert torch.equal(_bits(out), _bits(full))
    # all 32 channels of the limit in one launch
    table = [sig(f"S{k}", 11, -100.0 - k, 100.0 + 3 * k) for k in range(MAX_CHANNELS)]
    _, payload, records, R, n, off, gain, offset, ref = build(_case(table, 3))
    y = torch.ops.eeg_dcrnn.edf_decode(_bytes_tensor(payload, device), records, R, n, off, gain, offset, torch.float64)
    assert torch.equal(y.cpu(), torch.from_numpy(ref))


def check_golden_device(device):
    """the committed file through decode_edf (as a path): the stored float64 arrays, and their float32 rounding"""
    from eeg_gnn_ssl_amd import decode_edf
    with np.load(TINY_NPZ) as z:
        want, fs = z["physical"], float(z["sample_freq"])
    for dtype in (torch.float64, torch.float32):
        y, rate, header = decode_edf(TINY_EDF, ["EEG FP1", "EEG FP2", "EEG F3"], dtype=dtype, device=device)
        assert rate == fs and header.labels[0] == "EDF Annotations"
        assert torch.equal(y.cpu(), _want(want, dtype))


def check_large_index(device):
    """GPU: r * R passes 2^31 int16 (a payload above 4 GiB): one channel of two samples per record deep inside records of 32 769 int16"""
    R, records, n, off = 32769, 65600, 2, 32766
    assert (records - 1) * R > 2 ** 31 and 2 * records * R > 2 ** 32
    payload = torch.zeros(2 * records * R, dtype=torch.uint8, device=device)
    d = digital(5, records * n)
    payload.view(torch.int16).view(records, R)[:, off:off + n] = torch.from_numpy(d.reshape(records, n)).to(device)
    gain, offset = scaling(sig("A", n))
    want = np.float64(gain) * (np.float64(offset) + d.astype(np.float64))
    for dtype in (torch.float64, torch.float32):
        y = torch.ops.eeg_dcrnn.edf_decode(payload, records, R, n, [off], [gain], [offset], dtype)
        assert torch.equal(y.cpu(), _want(want[None], dtype)), dtype


def _call_c(lib, p, records, R, n, off, gain, offset, out, payload_bytes=None, out_stride=None, channels=None, payload_ptr=None, out_ptr=None, null=None):
    """the C entry as it is (no Python refusals in front); returns its status"""
    import ctypes
    from eeg_gnn_ssl_amd.ops import _p, _stream
    C = len(off)
    args = dict(payload=_p(p) if payload_ptr is None else ctypes.c_void_p(payload_ptr), chan_off=(ctypes.c_int64 * C)(*off), gain=(ctypes.c_double * C)(*gain),
                offset=(ctypes.c_double * C)(*offset), out=_p(out) if out_ptr is None else ctypes.c_void_p(out_ptr))
    if null is not None:
        args[null] = None
    return lib.query("eeg_dcrnn_edf_decode", args["payload"], p.numel() if payload_bytes is None else payload_bytes, records, R, n,
                     C if channels is None else channels, args["chan_off"], args["gain"], args["offset"], 1 if out.dtype == torch.float64 else 0,
                     args["out"], out.stride(0) if out_stride is None else out_stride, _stream(p))


def check_refusals(device):
    """every ValueError of the operator and of the chain, by message and BEFORE any launch (the event recorder sees none); the C entry
    refuses the same with an error code and names the argument"""
    from parity_suite import kernels_run
    from eeg_gnn_ssl_amd import RecordingDataset, _lib, decode_edf, load_edf_recordings, ops
    lib = _lib.get_lib()
    case = cases()["n3"]
    file, payload, records, R, n, off, gain, offset, ref = build(case)
    C, L = len(off), records * n
    p = _bytes_tensor(payload, device)
    odd = _bytes_tensor(b"\x00" + payload, device)[1:]
    out = _nan(C, L, device=device, dtype=torch.float64)
    op = torch.ops.eeg_dcrnn.edf_decode
    into = ops.edf_decode_into
    two = write_edf([sig("A-REF", 250), sig("B-REF", 256)], 2)
    short = write_edf([sig("A-REF", 125), sig("B-REF", 125)], 1, record_duration=0.5)

    def refused():
        for fn, text in (
                (lambda: op(p.view(torch.int16), records, R, n, off, gain, offset), r"payload must be a 1-D contiguous torch.uint8 tensor"),
                (lambda: op(p[None], records, R, n, off, gain, offset), r"payload must be a 1-D contiguous torch.uint8"),
                (lambda: op(p[::2], records, R, n, off, gain, offset), r"payload must be a 1-D contiguous torch.uint8"),
                (lambda: op(odd, records, R, n, off, gain, offset), r"payload starts at an odd address"),
                (lambda: op(p, 0, R, n, off, gain, offset), r"num_records=0 must be an integer >= 1"),
                (lambda: op(p, records, 0, n, off, gain, offset), r"R=0 must be an integer >= 1"),
                (lambda: op(p, records, R, 0, off, gain, offset), r"n=0 must be an integer >= 1"),
                (lambda: op(p, records, R, (1 << 30) + 1, off, gain, offset), r"n=1073741825 samples per record; 1\.\.1073741824"),
                (lambda: op(p, records, R, n, [], [], []), r"0 channels; 1\.\.32 \(EEG_EDF_MAX_CHANNELS\)"),
                (lambda: op(p, records, R, n, [0] * 33, [1.0] * 33, [0.0] * 33), r"33 channels; 1\.\.32"),
                (lambda: op(p, records, R, n, off, gain[:2], offset), r"2 gains and 3 offsets for 3 channels"),
                (lambda: op(p, records, R, n, off, gain, offset + [0.0]), r"3 gains and 4 offsets for 3 channels"),
                (lambda: op(p, records, R, n, [R - n + 1, 0, 0], gain, offset), rf"chan_off\[0\]={R - n + 1} \+ n=3 lies outside a record of R={R}"),
                (lambda: op(p, records, R, n, [0, -1, 0], gain, offset), r"chan_off\[1\]=-1 \+ n=3 lies outside"),
                (lambda: op(p, records, R, n, off, [1.0, float("nan"), 1.0], offset), r"gain\[1\]=nan must be a finite number"),
                (lambda: op(p, records, R, n, off, gain, [float("inf"), 0.0, 0.0]), r"offset\[0\]=inf must be a finite number"),
                (lambda: op(p, records + 1, R, n, off, gain, offset), rf"payload of {len(payload)} bytes is shorter than num_records=6 whole records"),
                (lambda: op(p[:-1], records, R, n, off, gain, offset), rf"payload of {len(payload) - 1} bytes is shorter"),
                (lambda: op(p, records, R, n, off, gain, offset, torch.float16), r"out_dtype=torch.float16; torch.float64 or torch.float32"),
                (lambda: into(p, records, R, n, off, gain, offset, out.half()), r"out must be a 2-D .* torch.float64 or torch.float32"),
                (lambda: into(p, records, R, n, off, gain, offset, out[0]), r"out must be a 2-D"),
                (lambda: into(p, records, R, n, off, gain, offset, out[:2]), rf"out is \(2, {L}\)"),
                (lambda: into(p, records, R, n, off, gain, offset, out[:, :-1]), rf"out is \(3, {L - 1}\)"),
                (lambda: into(p, records, R, n, off, gain, offset, out.t().contiguous().t()), r"rows of out must be contiguous"),
                (lambda: into(p, records, R, n, off, gain, offset, out[:1].expand(C, L)), r"row stride of at least the row length"),
                (lambda: into(p, records, R, n, off, gain, offset, torch.empty(C, L, dtype=torch.float64, device="meta")), r"out is .* on meta"),
                (lambda: into(p, True, R, n, off, gain, offset, out), r"num_records=True must be an integer"),
                (lambda: into(p, records, R, 2.0, off, gain, offset, out), r"n=2.0 must be an integer"),
                (lambda: into(p, records, R, n, [0.0, 1, 2], gain, offset, out), r"chan_off\[0\]=0.0"),
                (lambda: into(p, records, R, n, off, ["1", 1.0, 1.0], offset, out), r"gain\[0\]='1' must be a finite number"),
                (lambda: decode_edf(file, ["A", "Z"], device=device), r"channel 'Z' is not among"),
                (lambda: decode_edf(two, ["A", "B"], device=device), r"channel 'B' has samples_per_record=256"),
                (lambda: decode_edf(file[:-2], ["A"], device=device), r"num_records=5 records of"),
                (lambda: decode_edf(write_edf(case["signals"], 0), ["A"], device=device), r"num_records=0: the file holds no data record"),
                (lambda: decode_edf(write_edf([sig(f"S{k}", 2) for k in range(33)], 1), [f"S{k}" for k in range(33)], device=device), r"33 channels; at most 32"),
                (lambda: load_edf_recordings([], device=device), r"no recordings"),
                (lambda: load_edf_recordings([two, two], ["A"], to_freq=0, device=device), r"to_freq=0 must be a finite positive"),
                (lambda: load_edf_recordings([two, short], ["A"], device=device), r"recording 1: 125 samples at 250.0 Hz are shorter than one second"),
                (lambda: load_edf_recordings([two, file[:300]], ["A"], device=device), r"header_bytes=1536, the file has 300 bytes"),
                (lambda: RecordingDataset.from_edf([], np.array([[0, 0, 400, 0]]), None, window=200, x_steps=2, device=device), r"no recordings"),
        ):
            with pytest.raises(ValueError, match=text):
                fn()
    assert kernels_run(refused) == {}, "a refused call launched a kernel"

    def c_refused():
        for kwargs, text in (
                (dict(null="payload"), r"edf_decode: null"), (dict(null="chan_off"), r"edf_decode: null"), (dict(null="gain"), r"edf_decode: null"),
                (dict(null="offset"), r"edf_decode: null"), (dict(null="out"), r"edf_decode: null"),
                (dict(payload_ptr=p.data_ptr() + 1), r"edf_decode: payload must be 2-byte aligned"),
                (dict(payload_bytes=len(payload) - 1), rf"edf_decode: payload_bytes={len(payload) - 1} below the 2 \* num_records \* R = 2 \* 5 \* {R} bytes"),
                (dict(payload_bytes=0), r"edf_decode: payload_bytes=0 below"),
                (dict(channels=0), r"edf_decode: channels=0 unsupported \(1\.\.32\)"),
                (dict(channels=33), r"edf_decode: channels=33 unsupported \(1\.\.32\)"),
                (dict(out_stride=L - 1), rf"edf_decode: out_stride={L - 1} below the row length num_records \* n = {L}"),
                (dict(out_ptr=out.data_ptr() + 4), r"edf_decode: out must be aligned to its element size"),
        ):
            assert _call_c(lib, p, records, R, n, off, gain, offset, out, **kwargs) != 0, kwargs
            assert re.search(text, lib.last_error()), (kwargs, lib.last_error())
        for args, text in (((records, R, n, [R - n + 1, 0, 0]), rf"edf_decode: chan_off\[0\]={R - n + 1} \+ n=3 outside a record of R={R}"),
                           ((records, R, n, [0, 0, -1]), r"edf_decode: chan_off\[2\]=-1 \+ n=3 outside"),
                           ((0, R, n, off), r"edf_decode: num_records=0"), ((-1, R, n, off), r"edf_decode: num_records=-1"),
                           ((records, R, 0, off), r"edf_decode: n=0 samples per record unsupported"),
                           ((records, R, (1 << 30) + 1, off), r"edf_decode: n=1073741825 samples per record unsupported"),
                           ((records, n - 1, n, off), r"edf_decode: R=2 int16 per record below n=3"),
                           ((1 << 62, R, n, off), r"edf_decode: payload_bytes=\d+ below"),
                           ((records + 1, R, n, off), r"edf_decode: payload_bytes=\d+ below")):
            assert _call_c(lib, p, args[0], args[1], args[2], args[3], gain, offset, out) != 0, args
            assert re.search(text, lib.last_error()), (args, lib.last_error())
    assert kernels_run(c_refused) == {}, "a refused C call launched a kernel"
    assert bool(torch.isnan(out).all()), "a refused call wrote"
    assert _call_c(lib, p, records, R, n, off, gain, offset, out) == 0 and torch.equal(out.cpu(), torch.from_numpy(ref))      # accepted, the same arguments run
    if lib.is_device_build:
        with pytest.raises(ValueError, match=r"payload is on cpu; eeg_gnn_ssl_amd runs only on an MI355X"):
            ops._impls["edf_decode"](p.cpu(), records, R, n, off, gain, offset)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _e2e_files():
    """three synthetic files of the 19 channels: 250 Hz, 256 Hz with an odd extra signal in front, 200 Hz; 3 records of 1 s"""
    return [([sig(name + "-REF", 250, round(PMIN - k, 3), PMAX) for k, name in enumerate(CHANNELS)], list(range(19))),
            ([sig("EDF Annotations", 57, -1, 1, -32768, 32767)] + [sig(name + "-LE", 256) for name in reversed(CHANNELS)], [19 - k for k in range(19)]),
            ([sig(name + "-REF", 200, PMAX, PMIN) for name in CHANNELS] + [sig("EEG A1-REF", 200)], list(range(19)))]


def check_end_to_end(device):
    """`RecordingDataset.from_edf` over the three files against `from_native_rate` fed the restatement's float64 arrays and rates:
    the same resampler on the same inputs, so `signals` and `rec_table` are torch.equal, and one gather from each returns equal batches"""
    from eeg_gnn_ssl_amd import EpochSampler, RecordingDataset, load_edf_recordings
    files, recs, freqs = [], [], []
    for signals, picked in _e2e_files():
        file = write_edf(signals, 3)
        R, n, off, gain, offset = layout(signals, picked)
        recs.append(restate(file[256 * (len(signals) + 1):], 3, R, n, off, gain, offset))
        freqs.append(float(n))
        files.append(file)
    assert freqs == [250.0, 256.0, 200.0]
    table = np.array([[0, 0, 400, 0], [1, 200, 400, 0], [2, 200, 400, 0], [0, 200, 400, 0], [2, 0, 400, 0], [1, 0, 400, 0]], dtype=np.int64)
    y = torch.arange(len(table), dtype=torch.float32, device=device)
    window, x_steps = 200, 2
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, file in enumerate(files):
            paths.append(os.path.join(tmp, f"rec{k}.edf"))
            with open(paths[-1], "wb") as f:
                f.write(file)
        sources = [paths[0], files[1], np.frombuffer(files[2], dtype=np.uint8)]          # a path, bytes, a uint8 array
        ds = RecordingDataset.from_edf(sources, table, y, window=window, x_steps=x_steps, device=device)
        signals, rec_table, info = load_edf_recordings(paths, device=device)
    want = RecordingDataset.from_native_rate(recs, freqs, table, y, window=window, x_steps=x_steps, device=device)
    assert ds.N == 19 and ds.rec_table[:, 2].tolist() == [600, 600, 600]
    assert torch.equal(ds.rec_table, want.rec_table) and torch.equal(_bits(ds.signals), _bits(want.signals))
    assert torch.equal(rec_table, want.rec_table) and torch.equal(_bits(signals), _bits(want.signals))
    assert [(i["sample_freq"], i["samples"], i["resampled"]) for i in info] == [(250.0, 750, 600), (256.0, 768, 600), (200.0, 600, 600)]
    assert info[1]["header"].labels[0] == "EDF Annotations"
    # the file at 200 Hz is the restatement rounded once
    off, stride, samples = want.rec_table[2].tolist()
    assert torch.equal(ds.signals[off:off + 19 * stride].view(19, stride)[:, :samples].cpu(), torch.from_numpy(recs[2].astype(np.float32)))
    batches = []
    for d in (ds, want):
        sampler = EpochSampler(len(table), len(table), 7, 0, 1, device=device)           # no epoch begun: the identity permutation
        x_out = _nan(len(table), 19, x_steps * window, device=device, dtype=torch.float32)
        y_out = _nan(len(table), device=device, dtype=torch.float32)
        len_out = torch.zeros(len(table), dtype=torch.int64, device=device)
        d.gather(sampler, x_out, y_out, len_out)
        batches.append((x_out, y_out, len_out))
    for a, b in zip(*batches):
        assert torch.equal(a, b)
    assert torch.equal(batches[0][1], y) and bool(torch.isfinite(batches[0][0]).all())


def check_pyedflib(device):
    """where pyedflib exists: the committed file and a TUSZ-like one against EdfReader.readSignal"""
    pyedflib = pytest.importorskip("pyedflib")
    from eeg_gnn_ssl_amd import decode_edf
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t33.edf")
        case = cases()["tusz33"]
        with open(path, "wb") as f:
            f.write(write_edf(case["signals"], case["num_records"]))
        for file, names, picked in ((path, CHANNELS, case["picked"]), (TINY_EDF, ["EEG FP1", "EEG FP2", "EEG F3"], [1, 2, 3])):
            y, _, _ = decode_edf(file, names, device=device)
            reader = pyedflib.EdfReader(file)
            try:
                want = np.stack([reader.readSignal(s) for s in picked])
            finally:
                reader.close()
            assert torch.equal(y.cpu(), torch.from_numpy(want))


if __name__ == "__main__":
    import sys
    if "--write-golden" in sys.argv:
        write_golden()
        print("wrote", TINY_EDF, TINY_NPZ, TINY_TSE)
