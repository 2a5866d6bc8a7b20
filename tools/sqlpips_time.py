#!/usr/bin/env python3
"""SqueezeNet-LPIPS at the PIE-Bench shape (512 x 512), warm, device events around the native call on images already on
the device:

  native       hedit.lpips_score.NativeSqueezeLpips.distance (csrc/sqlpips.hip), stand-in weights, N pairs per call
  vgg source   (the only yardstick the library had) hedit_lpips_source of the face task's VGG16 LPIPS (csrc/lpips.hip) on
               TWO 512 x 512 images: the feature pass alone, no distance

for N = 1 / 3 / 16 pairs: `--repeats` timings, every figure the mean of enough back-to-back calls to fill `--window`
seconds (at least `--reps`); one JSON line per N with every repeat, the median and the spread (max - min).  `--count`
adds the number of kernel launches of one native call (torch.profiler); `--native-only K` runs nothing but K native calls
at the first N after one warm-up (for `rocprofv3 --kernel-trace --stats -- python tools/sqlpips_time.py --native-only 10`).

    python tools/sqlpips_time.py [--pairs 1 3 16] [--size 512] [--repeats 5] [--window 0.5] [--count] [--no-vgg]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib  # noqa: E402
from hedit.lpips_score import NativeSqueezeLpips  # noqa: E402


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


def vgg_source(dev, S):
    """a closure running hedit_lpips_source on two S x S images"""
    from hedit.arcface.lpips_loss import LPIPS_Loss
    m = LPIPS_Loss(src=torch.zeros(2, 3, S, S), device=dev, seed=0)
    h = m._native(dev)
    lib = m._lib
    x = torch.rand(2, 3, S, S, device=dev) * 2 - 1
    feats = torch.empty(2, lib.hedit_lpips_feature_floats(S, S), device=dev)
    ws = m._workspace(2, S, S, dev)

    def run():
        _lib.check(lib.hedit_lpips_source(h, _lib.ptr(x), 2, S, S, _lib.ptr(feats), _lib.ptr(ws), ws.numel(), _lib.cur_stream()))
    run.keep = (m, x, feats, ws)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 3, 16])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--no-vgg", action="store_true")
    ap.add_argument("--native-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S = a.size
    native = NativeSqueezeLpips(device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(1)

    def pair(N):
        x = torch.rand(N, 3, S, S, generator=g, device=dev) * 2 - 1
        return x, (x + 0.1 * torch.randn(N, 3, S, S, generator=g, device=dev)).clamp(-1, 1)

    if a.native_only:
        x, y = pair(a.pairs[0])
        native.distance(x, y)
        torch.cuda.synchronize()
        for _ in range(a.native_only):
            native.distance(x, y)
        torch.cuda.synchronize()
        return
    old = None if a.no_vgg else vgg_source(dev, S)
    for N in a.pairs:
        x, y = pair(N)
        new = lambda: native.distance(x, y)                              # noqa: E731
        for _ in range(2):
            new()
            if old is not None:
                old()
        rn = reps_for(new, a.window, a.reps)
        ro = reps_for(old, a.window, a.reps) if old is not None else 0
        tn, to = [], []
        for _ in range(a.repeats):
            tn.append(timed(new, rn))
            if old is not None:
                to.append(timed(old, ro))
        rec = {"pairs": N, "size": S, "calls_per_timing": rn, "native_ms_per_call": [round(t, 4) for t in tn],
               "native_median": round(statistics.median(tn), 4), "native_spread": round(max(tn) - min(tn), 4),
               "workspace_MiB": round(native._ws.numel() / 2 ** 20, 1)}
        if old is not None:
            rec.update({"vgg_source_2_images_ms_per_call": [round(t, 4) for t in to], "vgg_source_calls_per_timing": ro,
                        "vgg_source_median": round(statistics.median(to), 4), "vgg_source_spread": round(max(to) - min(to), 4)})
        if a.count:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                new()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            names = {}
            for e in ev:
                k = e.name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
                names[k] = names.get(k, 0) + 1
            rec["native_launches"] = len(ev)
            rec["native_launches_by_kernel"] = names
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
