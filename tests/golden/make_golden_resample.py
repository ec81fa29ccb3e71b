#!/usr/bin/env python3
"""Generates tests/golden/golden_resample_v1.npz from the genuine reference (run in the build container only; /root/reference never
travels): data/data_utils.py:158-170 `resampleData`, called as data/resample_signals.py:38-43 calls it (float64 signals,
window_size = int(samples / sample_freq)), on the small cases of tests/resample_suite.py at 2 channels.
Only OUTPUTS are stored (float64); the inputs are the closed form `resample_suite.signal`."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
from resample_suite import CASES, GOLDEN_CHANNELS, TO_FREQ, signal  # noqa: E402

for _m in ("h5py", "pyedflib"):
    sys.modules[_m] = types.ModuleType(_m)
sys.path.insert(0, REF)
from data.data_utils import resampleData  # noqa: E402

out = {}
for name, (nx, fs) in CASES.items():
    x = signal(GOLDEN_CHANNELS, nx)
    assert x.dtype == np.float64
    out[f"resample/{name}"] = np.asarray(resampleData(x, to_freq=TO_FREQ, window_size=int(x.shape[1] / fs)), dtype=np.float64)
np.savez_compressed(os.path.join(HERE, "golden_resample_v1.npz"), **out)
print({k: v.shape for k, v in out.items()})
