#!/usr/bin/env python3
"""hedit_attn_aggregate (csrc/step.hip) at the SD-1.5 shape, warm, on one GPU, beside the torch composition of
aggregate_attention on the same accumulators, alternating:

  cross16   the 16 x 16 cross maps of ("up", "down"): the layers store_layers reports with 256 tokens, 8 heads, 77 columns
  self32    the 32 x 32 self maps of ("up", "down"): the layers with 1024 tokens, 8 heads, 1024 columns

  native    one hedit_attn_aggregate launch over the selected buffers (both prompts of the pair); device events
  torch     what the reference composes from them for ONE prompt: item / cur_step, reshape, [select], cat, sum(0) / count --
            on the selected layers only (get_average_attention divides every stored layer); device events

`--repeats` timings per path, every figure the mean of enough back-to-back calls to fill `--window` seconds; one JSON line
per case with every repeat, the median, the spread (max - min), the bytes the reduction has to read and that over the
native median.  There is no gate.

    python tools/attn_aggregate_time.py [--images 1] [--repeats 5] [--window 0.5]
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
from hedit.unet import SD15_CONFIG, UNet2DConditionModel  # noqa: E402


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attn_aggregate_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    unet = UNet2DConditionModel(SD15_CONFIG, device=dev)          # geometry only: no weights are loaded
    layers = unet.store_layers(64, 64)
    heads, n, cur_step = unet.heads, a.images, 50
    g = torch.Generator(device=dev).manual_seed(0)
    for name, tokens, cols in (("cross16", 256, 77), ("self32", 1024, 1024)):
        picked = [i for place in ("up", "down") for i, (tok, pl) in enumerate(layers) if pl == place and tok == tokens]
        bufs = [torch.rand(n, 2, heads, tokens, cols, generator=g, device=dev) * cur_step for _ in picked]
        arr = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        out = torch.empty(n, 2, tokens, cols, device=dev)
        res = int(tokens ** 0.5)

        def native():
            _lib.check(lib.hedit_attn_aggregate(arr, len(bufs), heads, tokens, cols, n, cur_step, _lib.ptr(out), _lib.cur_stream()))

        def composed():
            maps = [(b[0].reshape(2 * heads, tokens, cols) / cur_step).reshape(2, -1, res, res, cols)[1] for b in bufs]
            m = torch.cat(maps, dim=0)
            return m.sum(0) / m.shape[0]

        paths = (("native", native), ("torch", composed))
        for _, fn in paths:
            for _ in range(3):
                fn()
        reps = {k: max(a.reps, int(a.window * 1000.0 / max(timed(fn, a.reps), 1e-3)) + 1) for k, fn in paths}
        times = {k: [] for k, _ in paths}
        for _ in range(a.repeats):
            for k, fn in paths:
                times[k].append(timed(fn, reps[k]))
        read = sum(b.numel() for b in bufs) * 4
        rec = {"case": name, "layers": len(bufs), "heads": heads, "tokens": tokens, "cols": cols, "images": n,
               "native_bytes_read": read, "torch_bytes_read_image_0": read // n}
        for k, _ in paths:
            t = times[k]
            rec.update({f"{k}_ms": [round(x, 4) for x in t], f"{k}_calls_per_timing": reps[k], f"{k}_median_ms": round(statistics.median(t), 4),
                        f"{k}_spread_ms": round(max(t) - min(t), 4)})
        rec["native_read_GBps"] = round(read / (rec["native_median_ms"] * 1e-3) / 1e9, 1)
        rec["max_abs_difference"] = float((out[0, 1].reshape(res, res, cols) - composed()).abs().max())
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
