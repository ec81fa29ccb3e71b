"""TUSZ files to clip tables: the front end of the reference's loaders (`data/data_utils.py` getEDFsignals / getOrderedChannels /
getSeizureTimes, `data/resample_signals.py`, the `file_markers_*` lists) without pyedflib or h5py.

Host (pure Python + numpy): `read_edf_header` parses the EDF header from the public specification, `select_channels` is the
reference's channel rule, `read_seizure_times` reads a `.tse_bi`, `read_markers_*` read the three marker-list formats and
`recording_ids` maps their names to indices, which feed `clip_table_detection / _ssl / _classification` unchanged.

Device: `decode_edf` uploads the PAYLOAD BYTES of a file (int16, a quarter of the float64 array a host reader materialises) and
decodes the selected channels with `torch.ops.eeg_dcrnn.edf_decode` (csrc/kernels_edf.h), EDFlib's arithmetic in float64.
`load_edf_recordings` chains that with the device resampler into the padded layout a `RecordingDataset` reads
(`RecordingDataset.from_edf`).

Two deliberate deviations from the reference: selected signals whose samples per record differ are refused (the
reference leaves such a row at zero through a swallowed exception), and the sampling rate is that of the SELECTED signals (the
reference reads signal 0's).  EDF+D, BDF and the EDF+ annotation signal's contents are out of scope."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

from . import ops, utils
from .resample import _check_freqs, _device, _target_length

_FIXED = (("version", 8), ("patient", 80), ("recording", 80), ("start_date", 8), ("start_time", 8), ("header_bytes", 8), ("reserved", 44),
          ("num_records", 8), ("record_duration", 8), ("ns", 4))
_PER_SIGNAL = (("label", 16), ("transducer", 80), ("physical_dimension", 8), ("physical_min", 8), ("physical_max", 8), ("digital_min", 8),
               ("digital_max", 8), ("prefilter", 80), ("samples_per_record", 8), ("signal_reserved", 32))


@dataclass
class EdfHeader:
    """the header of one EDF file; per-signal lists are in file order"""
    version: str
    patient: str
    recording: str
    start_date: str
    start_time: str
    header_bytes: int
    reserved: str
    num_records: int
    record_duration: float
    ns: int
    labels: List[str]
    nsamp: List[int]
    pmin: List[float]
    pmax: List[float]
    dmin: List[int]
    dmax: List[int]
    transducers: List[str]
    dimensions: List[str]
    prefilters: List[str]
    record_len: int                    # R: int16 per data record, the sum of nsamp
    payload_bytes: int                 # bytes behind the header

    def chan_off(self, s: int) -> int:
        """first int16 of signal s inside a data record"""
        return int(sum(self.nsamp[:s]))

    def gain_offset(self, s: int) -> Tuple[float, float]:
        """EDFlib's scaling of signal s, in float64: physical = gain * (offset + digital)"""
        gain = (np.float64(self.pmax[s]) - np.float64(self.pmin[s])) / (np.float64(self.dmax[s]) - np.float64(self.dmin[s]))
        return float(gain), float(np.float64(self.pmax[s]) / gain - np.float64(self.dmax[s]))


def _as_bytes(source) -> np.ndarray:
    """the whole file as a uint8 array (a path is read with numpy)"""
    if isinstance(source, (str, os.PathLike)):
        return np.fromfile(source, dtype=np.uint8)
    if isinstance(source, (bytes, bytearray, memoryview)):
        return np.frombuffer(source, dtype=np.uint8)
    if isinstance(source, np.ndarray) and source.dtype == np.uint8 and source.ndim == 1:
        return source
    raise ValueError(f"read_edf_header: source must be a path, bytes or a 1-D uint8 array, got {type(source).__name__}")


def _number(text: str, field: str, kind):
    try:
        return kind(text)
    except ValueError:
        raise ValueError(f"read_edf_header: {field}={text!r} is not a number") from None


def read_edf_header(source) -> EdfHeader:
    """the header of an EDF file (path, bytes or uint8 array), every refusal a ValueError that names the field"""
    raw = _as_bytes(source)
    if raw.size < 256:
        raise ValueError(f"read_edf_header: header_bytes: the file has {raw.size} bytes, the fixed header block alone has 256")
    fixed, at = {}, 0
    for name, width in _FIXED:
        fixed[name] = raw[at:at + width].tobytes().decode("ascii", errors="replace").strip()
        at += width
    if fixed["version"] != "0":
        raise ValueError(f"read_edf_header: version={fixed['version']!r}; only EDF (version '0') is read, not BDF or anything else")
    if fixed["reserved"].startswith("EDF+D"):
        raise ValueError("read_edf_header: reserved='EDF+D': discontinuous recordings are not supported (EDF and EDF+C are)")
    ns = _number(fixed["ns"], "ns", int)
    if ns < 1:
        raise ValueError(f"read_edf_header: ns={ns} signals (>= 1)")
    header_bytes = _number(fixed["header_bytes"], "header_bytes", int)
    if header_bytes != 256 * (ns + 1):
        raise ValueError(f"read_edf_header: header_bytes={header_bytes} for ns={ns} signals; 256 * (ns + 1) = {256 * (ns + 1)}")
    if raw.size < header_bytes:
        raise ValueError(f"read_edf_header: header_bytes={header_bytes}, the file has {raw.size} bytes")
    num_records = _number(fixed["num_records"], "num_records", int)
    record_duration = _number(fixed["record_duration"], "record_duration", float)
    if not record_duration > 0 or not np.isfinite(record_duration):
        raise ValueError(f"read_edf_header: record_duration={fixed['record_duration']!r} must be a positive number of seconds")
    cols = {}
    for name, width in _PER_SIGNAL:                                      # field-major: all labels, then all transducers, ...
        cols[name] = [raw[at + s * width:at + (s + 1) * width].tobytes().decode("ascii", errors="replace").strip() for s in range(ns)]
        at += ns * width
    num = lambda name, kind: [_number(t, f"{name}[{s}]", kind) for s, t in enumerate(cols[name])]     # noqa: E731
    nsamp, pmin, pmax = num("samples_per_record", int), num("physical_min", float), num("physical_max", float)
    dmin, dmax = num("digital_min", int), num("digital_max", int)
    for s in range(ns):
        if nsamp[s] < 1:
            raise ValueError(f"read_edf_header: samples_per_record[{s}]={nsamp[s]} (>= 1)")
        if dmax[s] == dmin[s]:
            raise ValueError(f"read_edf_header: digital_max[{s}] == digital_min[{s}] == {dmin[s]}: the signal has no scale")
    record_len = int(sum(nsamp))
    payload_bytes = int(raw.size - header_bytes)
    if num_records == -1:                                                # unknown: the whole records that are there
        num_records = payload_bytes // (2 * record_len)
    if num_records < 0:
        raise ValueError(f"read_edf_header: num_records={num_records} (>= 0, or -1 for unknown)")
    if payload_bytes < 2 * num_records * record_len:
        raise ValueError(f"read_edf_header: num_records={num_records} records of {2 * record_len} bytes need {2 * num_records * record_len} "
                         f"payload bytes, the file has {payload_bytes}")
    return EdfHeader(fixed["version"], fixed["patient"], fixed["recording"], fixed["start_date"], fixed["start_time"], header_bytes,
                     fixed["reserved"], num_records, record_duration, ns, cols["label"], nsamp, pmin, pmax, dmin, dmax, cols["transducer"],
                     cols["physical_dimension"], cols["prefilter"], record_len, payload_bytes)


def select_channels(header: EdfHeader, channels=None) -> List[int]:
    """signal indices of `channels` (default utils.INCLUDED_CHANNELS) by the reference's rule (data_utils.py getOrderedChannels): a
    label is cut at its first '-', the first signal that matches a name wins.  A missing channel and selected signals of different
    samples per record are refused."""
    channels = utils.INCLUDED_CHANNELS if channels is None else list(channels)
    if len(channels) < 1:
        raise ValueError("select_channels: no channels")
    labels = [label.split("-")[0] for label in header.labels]
    picked = []
    for ch in channels:
        if ch not in labels:
            raise ValueError(f"select_channels: channel {ch!r} is not among the file's labels {labels}")
        picked.append(labels.index(ch))
    n0 = header.nsamp[picked[0]]
    for ch, s in zip(channels, picked):
        if header.nsamp[s] != n0:
            raise ValueError(f"select_channels: channel {ch!r} has samples_per_record={header.nsamp[s]}, channel {channels[0]!r} has {n0}: "
                             f"the selected signals must share one sampling rate")
    return picked


def read_seizure_times(path) -> List[List[float]]:
    """[[start_s, end_s], ...] of the `.tse_bi` beside an `.edf` (or of the `.tse_bi` itself): every line that contains 'seiz'
    (the reference's getSeizureTimes)"""
    path = os.fspath(path)
    if not path.endswith(".tse_bi"):
        path = path.split(".edf")[0] + ".tse_bi"
    times = []
    with open(path) as f:
        for line in f:
            if "seiz" in line:
                fields = line.strip().split(" ")
                times.append([float(fields[0]), float(fields[1])])
    return times


def _marker_lines(path, what, fields):
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(",")
            if len(parts) != fields:
                raise ValueError(f"{what}: line {no} of {path}: {line!r} has {len(parts)} comma-separated fields, {fields} expected")
            rows.append((no, parts))
    return rows


def _clip_name(what, path, no, text):
    """'NAME.edf_K.h5' -> ('NAME.edf', K)"""
    stem, dot, ext = text.rpartition(".")
    name, sep, k = stem.rpartition("_")
    if ext != "h5" or not dot or not sep or not name.endswith(".edf") or not k.isdigit():
        raise ValueError(f"{what}: line {no} of {path}: {text!r} is not NAME.edf_K.h5")
    return name, int(k)


def _int_field(what, path, no, text):
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"{what}: line {no} of {path}: {text!r} is not an integer") from None


def read_markers_detection(path):
    """lines `NAME.edf_K.h5,label` -> (names, clip_idx int64, labels int64)"""
    what = "read_markers_detection"
    names, idx, labels = [], [], []
    for no, (clip, label) in _marker_lines(path, what, 2):
        name, k = _clip_name(what, path, no, clip)
        names.append(name)
        idx.append(k)
        labels.append(_int_field(what, path, no, label))
    return names, np.asarray(idx, dtype=np.int64), np.asarray(labels, dtype=np.int64)


def read_markers_ssl(path):
    """lines `NAME.edf_Kx.h5,NAME.edf_Ky.h5` -> (names, clip_idx_x int64, clip_idx_y int64); both halves name one recording"""
    what = "read_markers_ssl"
    names, kx, ky = [], [], []
    for no, (a, b) in _marker_lines(path, what, 2):
        name, x = _clip_name(what, path, no, a)
        name_y, y = _clip_name(what, path, no, b)
        if name_y != name:
            raise ValueError(f"{what}: line {no} of {path}: the input is a clip of {name!r}, the target of {name_y!r}")
        names.append(name)
        kx.append(x)
        ky.append(y)
    return names, np.asarray(kx, dtype=np.int64), np.asarray(ky, dtype=np.int64)


def read_markers_classification(path):
    """lines `NAME.edf,class,seizure_idx` -> (names, classes int64, seizure_idx int64)"""
    what = "read_markers_classification"
    names, classes, idx = [], [], []
    for no, (name, cls, k) in _marker_lines(path, what, 3):
        if not name.endswith(".edf"):
            raise ValueError(f"{what}: line {no} of {path}: {name!r} is not NAME.edf")
        names.append(name)
        classes.append(_int_field(what, path, no, cls))
        idx.append(_int_field(what, path, no, k))
    return names, np.asarray(classes, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def recording_ids(names, edf_paths) -> np.ndarray:
    """index into `edf_paths` of every recording name, matched by basename -> int64 (len(names),): the `rec_ids` of clip_table_*"""
    where = {}
    for r, p in enumerate(edf_paths):
        base = os.path.basename(os.fspath(p))
        if base in where:
            raise ValueError(f"recording_ids: edf_paths[{where[base]}] and edf_paths[{r}] share the basename {base!r}")
        where[base] = r
    ids = []
    for name in names:
        base = os.path.basename(name)
        if base not in where:
            raise ValueError(f"recording_ids: recording {base!r} is not among the {len(where)} edf_paths")
        ids.append(where[base])
    return np.asarray(ids, dtype=np.int64)


# ---- the device chain ----------------------------------------------------------------------------------------------------------
def _plan(what, source, channels):
    """(file bytes, header, picked signals, n, chan_off, gain, offset, sample_freq) of one file, every host refusal raised here"""
    raw = _as_bytes(source)
    header = read_edf_header(raw)
    picked = select_channels(header, channels)
    if len(picked) > ops.EDF_MAX_CHANNELS:
        raise ValueError(f"{what}: {len(picked)} channels; at most {ops.EDF_MAX_CHANNELS} are decoded")
    if header.num_records < 1:
        raise ValueError(f"{what}: num_records={header.num_records}: the file holds no data record")
    n = int(header.nsamp[picked[0]])
    scale = [header.gain_offset(s) for s in picked]
    return (raw, header, picked, n, [header.chan_off(s) for s in picked], [g for g, _ in scale], [o for _, o in scale],
            n / header.record_duration)


def _payload(raw, header) -> torch.Tensor:
    """the whole data records of the file as a host uint8 tensor (no copy, unless the source is read-only bytes)"""
    a = raw[header.header_bytes:header.header_bytes + 2 * header.num_records * header.record_len]
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def decode_edf(source, channels=None, dtype=torch.float64, device=None):
    """one EDF file (path, bytes or uint8 array) -> (signals (C, L) `dtype` on the device, sample_freq, header): the header is parsed on
    the host, the payload BYTES alone are uploaded and the selected channels decoded on the device, physical = gain * (offset + digital)
    in float64 as EDFlib's readSignal computes it (float32: that value rounded once).  L = num_records * samples per record."""
    what = "decode_edf"
    raw, header, _, n, chan_off, gain, offset, sample_freq = _plan(what, source, channels)
    payload = _payload(raw, header).to(_device(device))
    out = torch.ops.eeg_dcrnn.edf_decode(payload, header.num_records, header.record_len, n, chan_off, gain, offset, dtype)
    return out, sample_freq, header


def load_edf_recordings(paths, channels=None, to_freq=200, device=None):
    """EDF files -> (signals, rec_table, info) in the layout `resample_recordings` produces: one flat float32 buffer, recording r
    channel-major at rec_table[r] = (offset, stride, samples), offsets and strides padded to 4 floats, the padding zero.  Per file: the
    payload bytes go into ONE reused device byte buffer sized for the largest file, are decoded as float64 into ONE reused (C, L_max)
    staging buffer and resampled (`ops.resample_into`) straight into the file's place; a file already at `to_freq` is decoded as float32
    straight into its place.  info[r] = dict(sample_freq, samples, resampled, header)."""
    what = "load_edf_recordings"
    paths = list(paths)
    if len(paths) < 1:
        raise ValueError(f"{what}: no recordings")
    _check_freqs(what, 1.0, to_freq)
    plans, nums = [], []
    for r, p in enumerate(paths):
        plan = _plan(f"{what}: recording {r}", p, channels)
        header, n = plan[1], plan[3]
        nums.append(_target_length(f"{what}: recording {r}", header.num_records * n, plan[7], to_freq))
        plans.append(plan)
    dev = _device(device)
    C = len(plans[0][2])
    table, info, offset = [], [], 0
    for (_, header, _, n, _, _, _, fs), num in zip(plans, nums):
        native = header.num_records * n
        samples = native if num is None else num
        stride = -(-samples // 4) * 4
        table.append((offset, stride, samples))
        info.append(dict(sample_freq=fs, samples=native, resampled=samples, header=header))
        offset += C * stride
    signals = torch.zeros(offset, dtype=torch.float32, device=dev)
    bytes_buf = torch.empty(max(2 * p[1].num_records * p[1].record_len for p in plans), dtype=torch.uint8, device=dev)
    longest = max([p[1].num_records * p[3] for p, k in zip(plans, nums) if k is not None], default=0)
    staging = torch.empty(C * longest, dtype=torch.float64, device=dev) if longest else None
    for (raw, header, _, n, chan_off, gain, offs, _), num, (off, stride, samples) in zip(plans, nums, table):
        native = header.num_records * n
        payload = bytes_buf[:2 * header.num_records * header.record_len]
        payload.copy_(_payload(raw, header))
        place = signals[off:off + C * stride].view(C, stride)[:, :samples]
        if num is None:
            ops.edf_decode_into(payload, header.num_records, header.record_len, n, chan_off, gain, offs, place, what=what)
            continue
        x = staging[:C * native].view(C, native)
        ops.edf_decode_into(payload, header.num_records, header.record_len, n, chan_off, gain, offs, x, what=what)
        ops.resample_into(x, place, what=what)
    return signals, torch.tensor(table, dtype=torch.int64, device=dev), info
