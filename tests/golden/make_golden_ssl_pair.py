#!/usr/bin/env python3
"""Generates tests/golden/golden_ssl_pair_v1.npz from the genuine reference (run in the build container only;
/root/reference never travels): the pairing semantics of the SSL loader's augmentation --
  data/dataloader_ssl.py:159-171 `_random_reflect(EEG_seq, reflect=True/False)` on the input AND the target clip of one sample,
  data/dataloader_ssl.py:173-182 `_random_scale(EEG_seq, scale_factor=...)` (use_fft: += log(scale_factor)) on both with ONE factor,
  utils.py:393-428 `StandardScaler.transform` on both (dataloader_ssl.py:333-336), the target cut to its first output_len steps (:341),
  data/dataloader_ssl.py:184-233 `_get_indiv_graphs(eeg_clip_x, swap_nodes)`: the correlation graph of a reflected sample is built
  from the UN-reflected, un-scaled INPUT clip (its swapped name table is never read); the target plays no part in it.
Only inputs that are not closed-form and the OUTPUTS are stored."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
for _m in ("h5py", "pyedflib"):
    sys.modules[_m] = types.ModuleType(_m)
sys.path.insert(0, REF)
from constants import INCLUDED_CHANNELS  # noqa: E402
from data.data_utils import get_swap_pairs  # noqa: E402
from data.dataloader_ssl import SeizureDataset  # noqa: E402
from utils import StandardScaler  # noqa: E402


class _Self:
    """the attributes the methods under test read"""
    sensor_ids = [c.split(" ")[-1] for c in INCLUDED_CHANNELS]
    top_k = 3
    use_fft = True


me = _Self()
pairs = get_swap_pairs(INCLUDED_CHANNELS)
rng = np.random.RandomState(20261)
clip_x = rng.standard_normal((7, 19, 12)).astype(np.float64) * 1.5 + 3.0        # (T, N, D) log-amplitude-like features: the input
clip_y = rng.standard_normal((7, 19, 12)).astype(np.float64) * 1.5 + 3.0        # the following clip (the target is its first steps)
output_len, mean, std, scale = 3, 3.1, 1.45, 0.8625
scaler = StandardScaler(mean=mean, std=std)
out = {"pairs": np.asarray(pairs, dtype=np.int64), "clip_x": clip_x, "clip_y": clip_y, "output_len": np.array([output_len]),
       "mean_std": np.array([mean, std]), "scale": np.array([scale])}
for tag, reflect in (("reflected", True), ("plain", False)):
    # dataloader_ssl.py:317-341 with the two draws forced
    x_feature, swap_nodes = SeizureDataset._random_reflect(me, clip_x, reflect=reflect)
    y_feature, _ = SeizureDataset._random_reflect(me, clip_y, reflect=reflect)
    assert (swap_nodes is not None) == reflect
    x_feature = SeizureDataset._random_scale(me, x_feature, scale_factor=scale)
    y_feature = SeizureDataset._random_scale(me, y_feature, scale_factor=scale)
    out[f"{tag}/x"] = scaler.transform(x_feature)
    out[f"{tag}/y"] = scaler.transform(y_feature)[:output_len, :, :]
    out[f"{tag}/indiv_adj"] = SeizureDataset._get_indiv_graphs(me, clip_x, swap_nodes)
np.savez_compressed(os.path.join(HERE, "golden_ssl_pair_v1.npz"), **out)
print({k: getattr(v, "shape", None) for k, v in out.items()})
print("indiv graphs equal:", np.array_equal(out["plain/indiv_adj"], out["reflected/indiv_adj"]))
