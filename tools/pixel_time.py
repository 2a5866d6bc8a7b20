#!/usr/bin/env python3
"""The evaluator's pixel columns at the PIE-Bench shape (512 x 512), warm, on one GPU, native path and torch path in the
same run, alternating:

  native kernel   hedit.pixel_score.NativePixelMetrics.metrics (csrc/pixmetrics.hip) on N uint8 pairs and their masks already
                  on the device: the two launches of one call, all nine columns of every pair; device events
  native scores   NativePixelMetrics.scores on the same N pairs as host arrays: upload, the call, the 3 x 3 results back on
                  the host -- what the evaluator's --native_pixel --batch N pays per group; device events around work that
                  ends in the copy back
  torch           evaluation.MetricsCalculator("cuda") as the evaluator calls it without --native_pixel: for each of the N
                  pairs the nine columns one by one (whole / unedit / edit x mse / psnr / ssim), each its own upload,
                  its launches and its .item(); device events around work that ends in the last .item()

for N = 1 and 16: `--repeats` timings per path, every figure the mean of enough back-to-back calls to fill `--window`
seconds (at least `--reps`); one JSON line per N with every repeat, the median and the spread (max - min).  There is no gate.

    python tools/pixel_time.py [--pairs 1 16] [--size 512] [--repeats 5] [--window 0.5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from evaluation import evaluation as EV  # noqa: E402
from hedit.pixel_score import NativePixelMetrics  # noqa: E402


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def reps_for(fn, window, least):
    """calls that fill `window` seconds, from one timed probe of `least` calls"""
    ms = timed(fn, least)
    return max(least, int(window * 1000.0 / max(ms, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pixel_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    S = a.size
    native = NativePixelMetrics(device=dev)
    mc = EV.MetricsCalculator("cuda")
    rng = np.random.default_rng(1)
    for N in a.pairs:
        src = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
        tgt = np.clip(src.astype(np.int16) + rng.integers(-20, 21, src.shape), 0, 255).astype(np.uint8)
        mask = np.zeros((N, S, S), dtype=np.uint8)
        mask[:, S // 4:(3 * S) // 4, S // 5:(4 * S) // 5] = 1
        m3 = [m[:, :, None].repeat(3, axis=2).astype(np.float64) for m in mask]                  # as the evaluator's main builds it
        d = [torch.from_numpy(x).to(dev) for x in (src, tgt, mask)]
        items = [(src[i], tgt[i], mask[i], mask[i]) for i in range(N)]

        def kernel():
            native.metrics(d[0], d[1], d[2], d[2])

        def scores():
            native.scores(items)

        def torch_path():
            for i in range(N):
                for ma in (None, 1 - m3[i], m3[i]):
                    mc.calculate_mse(src[i], tgt[i], ma, ma)
                    mc.calculate_psnr(src[i], tgt[i], ma, ma)
                    mc.calculate_ssim(src[i], tgt[i], ma, ma)

        paths = (("native_kernel", kernel), ("native_scores", scores), ("torch", torch_path))
        for _, fn in paths:
            for _ in range(2):
                fn()
        reps = {name: reps_for(fn, a.window, a.reps) for name, fn in paths}
        times = {name: [] for name, _ in paths}
        for _ in range(a.repeats):
            for name, fn in paths:
                times[name].append(timed(fn, reps[name]))
        rec = {"pairs": N, "size": S, "columns_per_pair": 9}
        for name, _ in paths:
            t = times[name]
            rec.update({f"{name}_ms_per_call": [round(x, 4) for x in t], f"{name}_calls_per_timing": reps[name],
                        f"{name}_median": round(statistics.median(t), 4), f"{name}_spread": round(max(t) - min(t), 4)})
        # the two paths on the same pair, for the record: the largest difference per metric over the N pairs and the three parts
        got = np.stack(native.scores(items))
        worst = [0.0, 0.0, 0.0]
        for i in range(min(N, 2)):
            for p, ma in ((0, None), (1, m3[i]), (2, 1 - m3[i])):
                t = (mc.calculate_mse(src[i], tgt[i], ma, ma), mc.calculate_psnr(src[i], tgt[i], ma, ma), mc.calculate_ssim(src[i], tgt[i], ma, ma))
                e = (abs(got[i, p, 0] - t[0]) / t[0], abs(got[i, p, 1] - t[1]), abs(got[i, p, 2] - t[2]))
                worst = [max(w, float(x)) for w, x in zip(worst, e)]
        rec["native_vs_torch_cuda"] = {"mse_relative": worst[0], "psnr_dB": worst[1], "ssim_absolute": worst[2]}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
