#!/usr/bin/env python3
"""Prompt encoding at SD-1.x shape (768 wide, 12 layers, 12 heads, 49408 tokens, 77 positions), warm, device events around
the whole of HEditEngine.encode's work (tokenizer, upload, encoder):

  torch    the path without --native_text: the torch stand-in module on PyTorch-ROCm, prompt by prompt, each a batch of one
  native   hedit.text.NativeClipText (csrc/text.hip): ONE call for all prompts

for 3 prompts (one image: null, source, target) and 49 (a lock-step group of 24 images).  The two are measured alternately
in one process, `--repeats` times each (every figure the mean of `--reps` back-to-back calls); one JSON line per prompt
count with every repeat, the medians and the spread (max - min) of each side.  `--count` adds the number of kernel
launches of one native call (torch.profiler); `--native-only N` runs nothing but N native calls of 3 prompts after one
warm-up (for `rocprofv3 --kernel-trace --stats -- python tools/text_time.py --native-only 10`).

    python tools/text_time.py [--prompts 3 49] [--repeats 5] [--reps 10] [--count]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit.text import ClipTextEncoder, NativeClipText, WordTokenizer  # noqa: E402
from hedit import _lib  # noqa: E402
if os.environ.get("HEDIT_LIB_VARIANT"):       # tools/build_variant.sh side library (A/B runs inside one GPU call)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"lib_{os.environ['HEDIT_LIB_VARIANT']}.so.bin")

WORDS = "a photo of the cat dog sitting on bench red blue car road tall tree in with and river house".split()


def prompts(n):
    out = [""]
    for i in range(1, n):
        k = 3 + (i * 7) % 12
        out.append(" ".join(WORDS[(i * 5 + j * 3) % len(WORDS)] for j in range(k)))
    return out


def encode_loop(tok, enc, ps, dev):
    """HEditEngine.encode for a torch module"""
    out = []
    for p in ps:
        t = tok([p], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        with torch.no_grad():
            out.append(enc(t.input_ids.to(dev))[0].float())
    return torch.cat(out)


def encode_native(tok, enc, ps, dev):
    """HEditEngine.encode for a batch-invariant encoder"""
    t = tok(list(ps), padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
    return enc(t.input_ids)[0].float()


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
    ap.add_argument("--prompts", type=int, nargs="+", default=[3, 49])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--native-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    standin = ClipTextEncoder(seed=7).to(dev)
    native = NativeClipText.from_standin(standin)
    tok = WordTokenizer(stable_ids=True)
    tok.prescan(prompts(max(a.prompts)))
    if a.native_only:
        ps = prompts(3)
        encode_native(tok, native, ps, dev)
        torch.cuda.synchronize()
        for _ in range(a.native_only):
            encode_native(tok, native, ps, dev)
        torch.cuda.synchronize()
        return
    for n in a.prompts:
        ps = prompts(n)
        old, new = (lambda: encode_loop(tok, standin, ps, dev)), (lambda: encode_native(tok, native, ps, dev))
        err = float(((new() - old()).double().norm() / old().double().norm()).item())
        for _ in range(2):
            old(), new()
        to, tn = [], []
        for _ in range(a.repeats):
            to.append(timed(old, a.reps))
            tn.append(timed(new, a.reps))
        rec = {"prompts": n, "reps": a.reps, "torch_ms": [round(t, 3) for t in to], "native_ms": [round(t, 3) for t in tn],
               "torch_median_ms": round(statistics.median(to), 3), "native_median_ms": round(statistics.median(tn), 3),
               "torch_spread_ms": round(max(to) - min(to), 3), "native_spread_ms": round(max(tn) - min(tn), 3),
               "speedup": round(statistics.median(to) / statistics.median(tn), 2), "rel_l2_native_vs_torch": float(f"{err:.3e}")}
        if a.count:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                new()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            rec["native_launches"] = len(ev)
            names = {}
            for e in ev:
                k = e.name.split("(")[0].split("<")[0]
                names[k] = names.get(k, 0) + 1
            rec["native_launches_by_kernel"] = names
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
