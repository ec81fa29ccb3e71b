#!/usr/bin/env python3
"""Generates tests/golden/golden_varlen_v1.npz from the genuine reference (run in the build container only; /root/reference never
travels): the classification loader's variable-length sample, `data/dataloader_classification.py` `SeizureDataset.__getitem__` through
its `preproc_dir` branch (:318-320) --
  :321-331 augmentation (`_random_reflect`, `_random_scale` with use_fft: `+= log(scale)`) and `StandardScaler.transform` of the SHORT clip,
  :333-343 padding to max_seq_len with padding_val, `seq_len`,
  :356-361 `_get_indiv_graphs` of the unpadded, un-augmented, un-standardised clip and its dual random-walk supports.
The clip the stubbed `h5py.File` yields is `computeFFT` (data_utils.py:13-35) of every 200-sample step of the seeded signals below,
cut to curr_len steps.  The inputs are seeded (`signals`, repeated in tests/varlen_suite.py `varlen_signals`; the non-GPU test that
compares the suite's chain with this file fails if the two ever differ), so only OUTPUTS are stored."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
for _m in ("h5py", "pyedflib"):
    sys.modules[_m] = types.ModuleType(_m)
sys.path.insert(0, REF)
from data.data_utils import computeFFT  # noqa: E402
from data import dataloader_classification as dc  # noqa: E402
from utils import StandardScaler  # noqa: E402

MAX_SEQ_LEN, N, W, TOP_K = 4, 19, 200, 3
MEAN, STD, PADDING_VAL = 0.1, 1.3, 0
LENGTHS = (4, 3, 1)


def signals(seed, length):
    """(N, length) channel rows: the mix of make_golden_timedomain.py (five shared sources in 19 channels plus noise) at an amplitude
    that centres the log amplitudes near zero -- at the 30 of that file every log|FFT| row is ~6 plus noise, all cosines are ~0.99 and
    no clip has a top-k gap above 1e-4; here the rows differ by their channels' levels and the gaps reach 1e-2"""
    rs = np.random.RandomState(100 + seed)
    mix, src, noise = rs.standard_normal((N, 5)), rs.standard_normal((5, length)), rs.standard_normal((N, length))
    return 0.04 * (mix @ src + 0.7 * noise)


def fft_clip(raw, steps):
    """the preprocessed clip of `steps` steps: (steps, N, W/2) log amplitudes"""
    return np.stack([computeFFT(raw[:, t * W:(t + 1) * W], n=W)[0] for t in range(steps)], axis=0)


def topk_gap(clip):
    """smallest distance, over the rows of |corr|, between the last entry keep_topk keeps and the first it drops"""
    rows = clip.transpose(1, 0, 2).reshape(N, -1)
    corr = np.abs((rows @ rows.T) / np.sqrt(np.outer((rows * rows).sum(1), (rows * rows).sum(1))))
    np.fill_diagonal(corr, -1.0)
    srt = -np.sort(-corr, axis=1)
    return float((srt[:, TOP_K - 1] - srt[:, TOP_K]).min())


class _File:
    """stands in for h5py.File(<preproc_dir>/<edf>_<idx>.h5): hf['clip'][()] is the clip handed over"""
    clip = None

    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return {"clip": {(): _File.clip}}

    def __exit__(self, *a):
        return False


dc.h5py.File = _File
ds = dc.SeizureDataset.__new__(dc.SeizureDataset)          # (__init__ walks the TUSZ tree and reads the file markers)
ds.__dict__.update(input_dir=None, raw_data_dir=None, time_step_size=1, max_seq_len=MAX_SEQ_LEN, standardize=True,
                   scaler=StandardScaler(mean=MEAN, std=STD), split="train", padding_val=PADDING_VAL, data_augment=True,
                   adj_mat_dir=None, graph_type="individual", top_k=TOP_K, filter_type="dual_random_walk", use_fft=True,
                   preproc_dir="preproc", edf_files=["/tusz/a.edf"], file_tuples=[["a.edf", 2, 0]], size=1,
                   sensor_ids=[c.split(" ")[-1] for c in dc.INCLUDED_CHANNELS])

out = {"shape": np.array([MAX_SEQ_LEN, N, W, TOP_K]), "mean_std": np.array([MEAN, STD]), "padding_val": np.array([PADDING_VAL]),
       "lengths": np.array(LENGTHS)}
for curr_len in LENGTHS:
    found = {}
    for seed in range(4000):                # per outcome of the coin, the first seed whose truncated clip has no near-tie
        np.random.seed(seed)
        coin = bool(np.random.choice([True, False]))
        tag = "reflected" if coin else "plain"
        if tag not in found and topk_gap(fft_clip(signals(seed, MAX_SEQ_LEN * W), curr_len)) >= 2e-3:
            found[tag] = seed
        if len(found) == 2:
            break
    assert set(found) == {"reflected", "plain"}, (curr_len, found)
    for tag, seed in sorted(found.items()):
        _File.clip = fft_clip(signals(seed, MAX_SEQ_LEN * W), curr_len)
        np.random.seed(seed)
        coin, factor = bool(np.random.choice([True, False])), float(np.random.uniform(0.8, 1.2))
        np.random.seed(seed)
        x, y, seq_len, supports, adj, name = ds[0]
        assert coin == (tag == "reflected") and int(seq_len) == curr_len and tuple(x.shape) == (MAX_SEQ_LEN, N, W // 2)
        gap = topk_gap(_File.clip)
        print(f"len {curr_len} {tag}: seed {seed}, factor {factor:.6f}, smallest top-k gap {gap:.2e}")
        assert gap >= 2e-3, gap
        key = f"len{curr_len}/{tag}"
        out[f"{key}/seed"] = np.array([seed])
        out[f"{key}/scale"] = np.array([factor])
        out[f"{key}/x"] = x.numpy()
        out[f"{key}/seq_len"] = seq_len.numpy()
        out[f"{key}/indiv_adj"] = np.asarray(adj)
        out[f"{key}/supports"] = np.stack([s.numpy() for s in supports])
np.savez_compressed(os.path.join(HERE, "golden_varlen_v1.npz"), **out)
print({k: getattr(v, "shape", None) for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "golden_varlen_v1.npz")))
