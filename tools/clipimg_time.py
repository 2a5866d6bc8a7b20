#!/usr/bin/env python3
"""The CLIP image tower at the ViT-L/14 shape (1024 wide, 24 layers, 16 heads, 257 tokens, embedding 768), warm, device
events around the encode call on preprocessed images already on the device:

  native        hedit.clip_score.NativeClipImage (csrc/clipimg.hip), stand-in weights generated on the device
  transformers  (for information) CLIPVisionModelWithProjection in fp32 on PyTorch-ROCm, same GPU, its own random weights

for batches of 1 / 8 / 32 images: `--repeats` timings of each side, every figure the mean of `--reps` back-to-back calls
divided by the batch (ms per image); one JSON line per batch with every repeat, the medians and the spread (max - min).
`--count` adds the number of kernel launches of one native call (torch.profiler); `--native-only N` runs nothing but N
native calls at the first batch size after one warm-up (for `rocprofv3 --kernel-trace --stats -- python
tools/clipimg_time.py --native-only 10`); `--no-hf` leaves transformers out.

    python tools/clipimg_time.py [--batches 1 8 32] [--repeats 5] [--reps 5] [--count] [--no-hf]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit.clip_score import NativeClipImage  # noqa: E402
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


def hf_tower(dev):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                         hidden_act="quick_gelu", projection_dim=768)
    return CLIPVisionModelWithProjection(c).eval().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--native-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    native = NativeClipImage.from_standin(device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    if a.native_only:
        x = torch.randn(a.batches[0], 3, 224, 224, generator=g, device=dev)
        native(x)
        torch.cuda.synchronize()
        for _ in range(a.native_only):
            native(x)
        torch.cuda.synchronize()
        return
    hf = None if a.no_hf else hf_tower(dev)
    for B in a.batches:
        x = torch.randn(B, 3, 224, 224, generator=g, device=dev)
        new = lambda: native(x)                                          # noqa: E731
        if hf is not None:
            def old():
                with torch.no_grad():
                    return hf(pixel_values=x).image_embeds
        for _ in range(2):
            new()
            if hf is not None:
                old()
        tn, to = [], []
        for _ in range(a.repeats):
            tn.append(timed(new, a.reps) / B)
            if hf is not None:
                to.append(timed(old, a.reps) / B)
        rec = {"batch": B, "reps": a.reps, "native_ms_per_image": [round(t, 3) for t in tn], "native_median": round(statistics.median(tn), 3),
               "native_spread": round(max(tn) - min(tn), 3)}
        if hf is not None:
            rec.update({"transformers_fp32_ms_per_image": [round(t, 3) for t in to], "transformers_median": round(statistics.median(to), 3),
                        "transformers_spread": round(max(to) - min(to), 3)})
        if a.count:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                new()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            rec["native_launches"] = len(ev)
            names = {}
            for e in ev:
                k = e.name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
                names[k] = names.get(k, 0) + 1
            rec["native_launches_by_kernel"] = names
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
