#!/usr/bin/env python3
"""Per-tensor mean / std of the reference's shipped correlation-graph SSL checkpoint (pretrained/pretrained_correlation_graph_12s.pth.tar,
2.7 MB of trained weights: too large to commit) -> pretrained_stats.json.  tests/test_pretrained_checkpoints.py rebuilds a
stand-in of that file from these figures and pretrained_manifest.json (names, shapes, shared decoder cells).
Run once, here:  python tests/golden/make_pretrained_stats.py --reference DIR"""
import argparse
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("pretrained_correlation_graph_12s.pth.tar",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (tsy935/eeg-gnn-ssl)")
    a = ap.parse_args()
    out = {}
    for name in NAMES:
        sd = torch.load(os.path.join(a.reference, "pretrained", name), map_location="cpu", weights_only=True)["model_state"]
        out[name] = {k: [round(float(v.double().mean()), 8), round(float(v.double().std()), 8)] for k, v in sorted(sd.items())}
    with open(os.path.join(HERE, "pretrained_stats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
