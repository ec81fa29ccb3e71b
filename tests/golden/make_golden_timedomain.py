#!/usr/bin/env python3
"""Generates tests/golden/golden_timedomain_v1.npz from the genuine reference (run in the build container only;
/root/reference never travels): the reference's time-domain input mode (`use_fft = False`) --
  data/dataloader_detection.py:233-256 `_random_reflect` / `_random_scale` (`EEG_seq *= scale_factor`) of the detection loader under
      a seeded `np.random` (the coin and the factor it drew are recorded),
  data/dataloader_ssl.py:159-182,317-341 the SSL loader with that coin and that factor forced on the input AND the target clip,
  utils.py:393-428 `StandardScaler.transform` on both, the target cut to its first output_len steps,
  data/dataloader_detection.py:258-307 `_get_indiv_graphs` of the un-augmented clip.
The clips are what `computeSliceMatrix(is_fft=False)` (dataloader_detection.py:25-85) returns for the seeded signals below:
clip[t, n, :] = raw[n, t*W:(t+1)*W].  The inputs are seeded (`signals`, repeated in tests/timedomain_suite.py: the non-GPU test that
compares the suite's chain with this file at 1e-12 fails if the two ever differ), so only OUTPUTS are stored."""
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
from data.dataloader_detection import SeizureDataset as DetectionDataset  # noqa: E402
from data.dataloader_ssl import SeizureDataset as SslDataset  # noqa: E402
from utils import StandardScaler  # noqa: E402

T, N, W, OUTPUT_LEN, TOP_K = 4, 19, 200, 2, 3
MEAN, STD = 1.7, 41.0


def signals(seed, length):
    """(N, length) channel rows: five shared sources mixed into 19 channels plus noise -- correlations of every size, and (asserted
    below) no near-tie at the top-k boundary of any row"""
    rs = np.random.RandomState(100 + seed)
    mix, src, noise = rs.standard_normal((N, 5)), rs.standard_normal((5, length)), rs.standard_normal((N, length))
    return 30.0 * (mix @ src + 0.7 * noise)


def windows(raw):
    """computeSliceMatrix(is_fft=False): np.stack of the (num_channels, 200) time steps"""
    return np.stack([raw[:, t * W:(t + 1) * W] for t in range(raw.shape[1] // W)], axis=0)


def topk_gap(clip):
    """smallest distance, over the rows of |corr|, between the last entry keep_topk keeps and the first it drops"""
    rows = clip.transpose(1, 0, 2).reshape(N, -1)
    corr = np.abs((rows @ rows.T) / np.sqrt(np.outer((rows * rows).sum(1), (rows * rows).sum(1))))
    np.fill_diagonal(corr, -1.0)
    srt = -np.sort(-corr, axis=1)
    return float((srt[:, TOP_K - 1] - srt[:, TOP_K]).min())


class _Self:
    """the attributes the methods under test read"""
    sensor_ids = [c.split(" ")[-1] for c in INCLUDED_CHANNELS]
    top_k = TOP_K
    use_fft = False


me = _Self()
scaler = StandardScaler(mean=MEAN, std=STD)
out = {"shape": np.array([T, N, W, OUTPUT_LEN, TOP_K]), "mean_std": np.array([MEAN, STD])}

found = {}
for seed in range(64):                      # per outcome of the detection loader's coin, the first seed whose clip has no near-tie
    np.random.seed(seed)
    coin = bool(np.random.choice([True, False]))
    if topk_gap(windows(signals(seed, 2 * T * W)[:, :T * W])) >= 2e-3:
        found.setdefault("reflected" if coin else "plain", seed)
assert set(found) == {"reflected", "plain"}
for tag, seed in sorted(found.items()):
    raw = signals(seed, 2 * T * W)          # the input clip and the clip that follows it
    clip_x, clip_y = windows(raw[:, :T * W]), windows(raw[:, T * W:])
    assert clip_x.shape == (T, N, W)
    # the draws of dataloader_detection.py:384-389 under this seed: `np.random.choice` of _random_reflect, then `np.random.uniform`
    np.random.seed(seed)
    coin, factor = bool(np.random.choice([True, False])), float(np.random.uniform(0.8, 1.2))
    np.random.seed(seed)
    x_det, swap_nodes = DetectionDataset._random_reflect(me, clip_x)
    x_det = DetectionDataset._random_scale(me, x_det)
    assert (swap_nodes is not None) == coin == (tag == "reflected")
    # dataloader_ssl.py:317-341 with these two draws forced
    x_ssl, swap_ssl = SslDataset._random_reflect(me, clip_x, reflect=coin)
    y_ssl, _ = SslDataset._random_reflect(me, clip_y, reflect=coin)
    x_ssl = SslDataset._random_scale(me, x_ssl, scale_factor=factor)
    y_ssl = SslDataset._random_scale(me, y_ssl, scale_factor=factor)
    assert np.array_equal(x_ssl, x_det), "the two loaders give one array for one pair of draws"
    adj = DetectionDataset._get_indiv_graphs(me, clip_x, swap_nodes)
    assert np.array_equal(adj, SslDataset._get_indiv_graphs(me, clip_x, swap_ssl))
    gap = topk_gap(clip_x)              # no near-tie where keep_topk cuts: an fp32 Gram may not move the pattern
    print(f"{tag}: seed {seed}, factor {factor:.6f}, smallest top-k gap {gap:.2e}")
    assert gap >= 1e-3, gap
    out[f"{tag}/seed"] = np.array([seed])
    out[f"{tag}/scale"] = np.array([factor])
    out[f"{tag}/x"] = scaler.transform(x_det)
    out[f"{tag}/y"] = scaler.transform(y_ssl)[:OUTPUT_LEN, :, :]
    out[f"{tag}/indiv_adj"] = adj
np.savez_compressed(os.path.join(HERE, "golden_timedomain_v1.npz"), **out)
print({k: getattr(v, "shape", None) for k, v in out.items()})
