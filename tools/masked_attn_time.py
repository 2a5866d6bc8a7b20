#!/usr/bin/env python3
"""Device time of the class-matched self-attention kernel (csrc/maskattn.hip) against the plain mutual self-attention kernel
(hedit_k_self_attn with kv_src, what a layer runs without masks), warm, device events around `--reps` back-to-back launches,
the candidates alternating in `--rounds` rounds (the median and the spread are reported).  Shapes: the three attention levels
of SD-1.5 at 64 x 64 latents, the 4 rows [x_orig|null, x_k|null, x_orig|src, x_k|tar].  The plain kernel cannot leave rows
out, so the comparison is made twice: kernel against kernel on all four rows (`masked_over_plain`), and the masked layer as
the executor runs it -- the two source rows on the plain kernel, the two target rows on the class-matched one -- against the
unmasked layer (`layer_new_over_parent`).  Masks: Bernoulli(0.5) (every key tile mixed, nothing skipped) and the upper half
plane for keys and queries (a block of 128 queries is pure and skips the key tiles of the other class: half of them).  Then
one SD-shaped UNet call (random weights, B = 4) under the plain editor's plan and under the mask-guided editor's.  One JSON
line per measurement.

    python tools/masked_attn_time.py [--reps 20] [--rounds 5] [--no-unet]
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

DEV = torch.device("cuda:0")


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def kernels(a):
    lib = _lib.lib()
    B, kv = 4, [0, 0, 2, 2]
    for heads, d, N in [(8, 40, 4096), (8, 80, 1024), (8, 160, 256)]:
        c = heads * d
        g = torch.Generator().manual_seed(N)
        qk = (torch.randn(B * N, 2 * c, generator=g) * 0.3).to(_lib.storage_dtype()).to(DEV)
        vt = torch.randn(c, B * N, generator=g).to(_lib.storage_dtype()).to(DEV)
        out = torch.empty(B * N, c, device=DEV, dtype=_lib.storage_dtype())
        kv_t = torch.tensor(kv, dtype=torch.int32, device=DEV)
        all_t = torch.arange(B, dtype=torch.int32, device=DEV)
        tar_t = torch.tensor([1, 3], dtype=torch.int32, device=DEV)

        def plain(b0=0, nb=B, kvp=kv_t):
            """hedit_k_self_attn on rows [b0, b0 + nb) (offset bases, as the executor launches the source rows)"""
            _lib.check(lib.hedit_k_self_attn(C.c_void_p(qk.data_ptr() + b0 * N * 2 * c * 2), 2 * c,
                                             C.c_void_p(qk.data_ptr() + (b0 * N * 2 * c + c) * 2), 2 * c,
                                             C.c_void_p(vt.data_ptr() + b0 * N * 2), B * N,
                                             C.c_void_p(out.data_ptr() + b0 * N * c * 2), c, nb, N, heads, d, None,
                                             _lib.ptr(kvp) if kvp is not None else None, None))

        upper = (torch.arange(N) < N // 2).to(torch.uint8).expand(B, N).contiguous()
        masks = {"bernoulli": ((torch.rand(B, N, generator=g) < 0.5).to(torch.uint8), (torch.rand(B, N, generator=g) < 0.5).to(torch.uint8)),
                 "half_plane": (upper, upper)}
        for name, (cq, ck) in masks.items():
            cq, ck = cq.to(DEV), ck.to(DEV)

            def masked(rows_t):
                _lib.check(lib.hedit_k_masked_self_attn(_lib.ptr(qk), 2 * c, C.c_void_p(qk.data_ptr() + c * 2), 2 * c, _lib.ptr(vt), B * N,
                                                        _lib.ptr(out), c, B, N, heads, d, _lib.ptr(rows_t), rows_t.numel(), _lib.ptr(kv_t),
                                                        _lib.ptr(cq), _lib.ptr(ck), None))

            def layer_new():      # what the executor runs in a masked layer: source rows plain, target rows class-matched
                plain(0, 1, None)
                plain(2, 1, None)
                masked(tar_t)

            cases = {"plain4": plain, "masked4": lambda: masked(all_t), "layer_new": layer_new}
            for f in cases.values():
                f()
            torch.cuda.synchronize()
            t = {k: [] for k in cases}
            for _ in range(a.rounds):
                for k, f in cases.items():
                    t[k].append(timed(f, a.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({"heads": heads, "d": d, "N": N, "mask": name, "storage": _lib.STORAGE,
                              "plain_4rows_us": round(med["plain4"], 1), "masked_4rows_us": round(med["masked4"], 1),
                              "layer_new_us": round(med["layer_new"], 1),
                              "masked_over_plain": round(med["masked4"] / med["plain4"], 3),
                              "layer_new_over_parent": round(med["layer_new"] / med["plain4"], 3),
                              "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()}}))


def unet_call(a):
    from hedit.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    from hedit.unet import UNet2DConditionModel
    unet = UNet2DConditionModel(device="cuda:0")
    unet.init_random(0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 4, 64, 64, generator=g).to(DEV)
    ctx = torch.randn(4, 77, 768, generator=g).to(DEV)
    m = torch.zeros(64, 64)
    m[16:48, 16:48] = 1
    eds = {"plain": MutualSelfAttentionControl(0, 10), "masked": MutualSelfAttentionControlMask(0, 10, mask_s=m, mask_t=m)}
    fs = {k: (lambda ed=ed: unet.forward_raw(x, 500.0, ctx, ed._plan(unet, 4, 64, 64, True))) for k, ed in eds.items()}
    for f in fs.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fs}
    for _ in range(a.rounds):
        for k, f in fs.items():
            t[k].append(timed(f, max(2, a.reps // 4)))
    p, mk = statistics.median(t["plain"]), statistics.median(t["masked"])
    print(json.dumps({"unet": "SD-1.5 shape, B=4, 64x64, layers >= 10", "storage": _lib.STORAGE, "plain_ms": round(p / 1e3, 3),
                      "masked_ms": round(mk / 1e3, 3), "masked_over_plain": round(mk / p, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-unet", action="store_true")
    a = ap.parse_args()
    kernels(a)
    if not a.no_unet:
        unet_call(a)


if __name__ == "__main__":
    main()
