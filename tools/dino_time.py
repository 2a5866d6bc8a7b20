#!/usr/bin/env python3
"""The Structure Distance at the PIE-Bench shape (512 x 512 -> 224 x 224, DINO ViT-B/8, keys of block 11), warm, device
events around the native call on images already on the device:

  native   hedit.dino_score.NativeDinoStructure.distance (csrc/dino.hip), stand-in weights, N pairs per call

for N = 1 / 8 pairs: `--repeats` timings, every figure the mean of enough back-to-back calls to fill `--window` seconds (at
least `--reps`); one JSON line per N with every repeat, the median and the spread (max - min).  `--count` adds the number of
kernel launches of one call and the device time per kernel class (torch.profiler: split = the fp32 -> split-bf16 operand
pass, gemm = the split-bf16 products, attention, selfsim = norms + Gram tiles + sum, other = preprocess / patches / tokens /
LayerNorm / bias adds / copies); `--native-only K` runs nothing but K calls at the first N after one warm-up (for
`rocprofv3 --kernel-trace --stats -- python tools/dino_time.py --native-only 10`).

    python tools/dino_time.py [--pairs 1 8] [--size 512] [--repeats 5] [--window 0.5] [--count] [--weights dino_vitbase8_pretrain.pth]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit.dino_score import NativeDinoStructure  # noqa: E402
from hedit import _lib  # noqa: E402
if os.environ.get("HEDIT_LIB_VARIANT"):       # tools/build_variant.sh side library (A/B runs inside one GPU call)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"lib_{os.environ['HEDIT_LIB_VARIANT']}.so.bin")


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


def kernel_class(name):
    n = name.lower()
    if "mfma_attn" in n:
        return "attention"
    if "selfsim" in n or "row_norm" in n:
        return "selfsim"
    if "split3" in n:
        return "split"
    if "gemm" in n or "splitk" in n or "reduce" in n:
        return "gemm"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--weights", type=str, default=None, help="a LOCAL DINO state dict instead of the stand-in ViT-B/8")
    ap.add_argument("--native-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S = a.size
    native = NativeDinoStructure(a.weights, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(1)

    def pair(N):
        x = torch.rand(N, 3, S, S, generator=g, device=dev) * 255
        return x, (x + 25 * torch.randn(N, 3, S, S, generator=g, device=dev)).clamp(0, 255)

    if a.native_only:
        x, y = pair(a.pairs[0])
        native.distance(x, y)
        torch.cuda.synchronize()
        for _ in range(a.native_only):
            native.distance(x, y)
        torch.cuda.synchronize()
        return
    n = native.net
    for N in a.pairs:
        x, y = pair(N)
        new = lambda: native.distance(x, y)                              # noqa: E731
        for _ in range(2):
            new()
        rn = reps_for(new, a.window, a.reps)
        tn = [timed(new, rn) for _ in range(a.repeats)]
        rec = {"pairs": N, "size": S, "width": n.width, "layers": n.layers, "key_layer": n.key_layer, "tokens": n.tokens, "calls_per_timing": rn,
               "native_ms_per_call": [round(t, 4) for t in tn], "native_median": round(statistics.median(tn), 4),
               "native_spread": round(max(tn) - min(tn), 4), "workspace_MiB": round(native._ws.numel() / 2 ** 20, 1)}
        if a.count:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                new()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            launches, ms = {}, {}
            for e in ev:
                k = kernel_class(e.name)
                launches[k] = launches.get(k, 0) + 1
                ms[k] = ms.get(k, 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) / 1000.0
            rec["native_launches"] = len(ev)
            rec["native_launches_by_class"] = launches
            rec["native_ms_by_class_under_the_profiler"] = {k: round(v, 4) for k, v in ms.items()}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
