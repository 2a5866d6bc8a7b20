#!/usr/bin/env python3
"""Device time of the face-swapping post-processing mask: FaceParsing labels + face_mask for 256 x 256 images
(csrc/faceparse.hip), warm, measured with device events around `--reps` back-to-back calls.  Prints one JSON line per batch size.

    python tools/faceparse_time.py [--batches 1 8] [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit.arcface import FaceParsing, face_mask  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    net = FaceParsing(device="cuda:0").init_random(0)
    g = torch.Generator().manual_seed(0)
    for B in a.batches:
        x = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
        for _ in range(3):
            face_mask(net(x))
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tl = torch.cuda.Event(enable_timing=True)
        ms_lab = ms_all = 0.0
        for _ in range(a.reps):
            t0.record()
            lab = net(x)
            tl.record()
            face_mask(lab)
            t1.record()
            t1.synchronize()
            ms_lab += t0.elapsed_time(tl)
            ms_all += t0.elapsed_time(t1)
        print(json.dumps({"B": B, "H": a.size, "W": a.size, "reps": a.reps, "labels_ms": round(ms_lab / a.reps, 4),
                          "labels_plus_mask_ms": round(ms_all / a.reps, 4), "per_image_ms": round(ms_all / a.reps / B, 4)}))


if __name__ == "__main__":
    main()
