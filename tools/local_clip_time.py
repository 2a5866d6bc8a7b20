#!/usr/bin/env python3
"""Two records for DESIGN.md section 1o, both wall clock around a synchronised call (the host work is part of what is measured):

  preprocess  512 x 512 -> 224 x 224 per image, from the uint8 array to the fp32 tensor ON THE DEVICE:
                host    hedit.clip_score.preprocess_pil per image (PIL bicubic + numpy), stacked, uploaded
                device  hedit.image_prep.NativeImagePrep (csrc/imgprep.hip): one uint8 upload, one native call
              (the two tensors are compared with torch.equal before anything is timed)
  local_clip  hedit.local_clip_score.NativeLocalClip at the ViT-L/14 stand-in shapes with T made-up templates, ms per pair,
              split into text (2 T prompts per pair through the text tower), image (preprocessing + image tower, two images
              per pair) and the head launch; every pair has its own two prompts, so nothing is saved by de-duplication

for each batch size: `--repeats` timings, each the mean of `--reps` calls; one JSON line per record with every repeat, the
median and the spread (max - min).

    python tools/local_clip_time.py [--batches 1 8] [--prep-batches 1 8 32] [--templates 80] [--repeats 5] [--reps 3] [--skip-metric]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit.clip_score import NativeClip, preprocess_pil  # noqa: E402
from hedit.image_prep import NativeImagePrep  # noqa: E402
from hedit.local_clip_score import NativeLocalClip, direction  # noqa: E402


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(name, ts):
    return {name: [round(t, 3) for t in ts], name + "_median": round(statistics.median(ts), 3), name + "_spread": round(max(ts) - min(ts), 3)}


def images(n, seed, side=512):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    base = ((xx + yy) * 255 // (2 * side - 2)).astype(np.int64)[..., None]
    return [np.clip(base // 2 + rng.integers(0, 128, (side, side, 3)), 0, 255).astype(np.uint8) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prep-batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--templates", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-metric", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prep = NativeImagePrep(dev)
    for B in a.prep_batches:
        imgs = images(B, B)
        host = lambda: torch.from_numpy(np.stack([preprocess_pil(im, 224) for im in imgs])).to(dev)      # noqa: E731
        device = lambda: prep(imgs, 224, "transformers")                                                   # noqa: E731
        assert torch.equal(host(), device())
        th, td = [], []
        for _ in range(a.repeats):
            th.append(wall(host, a.reps) / B)
            td.append(wall(device, a.reps) / B)
        rec = {"record": "preprocess", "batch": B, "reps": a.reps}
        rec.update(summary("host_ms_per_image", th))
        rec.update(summary("device_ms_per_image", td))
        print(json.dumps(rec), flush=True)
    if a.skip_metric:
        return
    clip = NativeClip.from_standin(device=dev)
    lc = NativeLocalClip(clip, [f"template number {i} of a {{}}." for i in range(a.templates)])
    words = "a photo painting sketch of the cat dog bird horse car house tree river on in under near bench field road".split()
    for B in a.batches:
        rng = np.random.default_rng(100 + B)
        prompts = [" ".join(rng.choice(words, 8)) + f" {k}" for k in range(2 * B)]
        imgs = images(2 * B, 50 + B)
        items = [(imgs[2 * k], prompts[2 * k], imgs[2 * k + 1], prompts[2 * k + 1]) for k in range(B)]
        text = lc._text(prompts)
        txt = torch.stack([torch.stack([text[it[1]], text[it[3]]]) for it in items])
        img = lc._images(imgs).reshape(B, 2, -1)
        lc.scores(items)
        parts = {"text": lambda: lc._text(prompts), "image": lambda: lc._images(imgs), "head": lambda: direction(txt, img),
                 "total": lambda: lc.scores(items)}
        rec = {"record": "local_clip", "pairs": B, "templates": a.templates, "reps": a.reps}
        for name, fn in parts.items():
            rec.update(summary(name + "_ms_per_pair", [wall(fn, a.reps) / B for _ in range(a.repeats)]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
