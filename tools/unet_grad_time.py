#!/usr/bin/env python3
"""Device time of the SD UNet's input-gradient pass at the SD-1.5 shape (csrc/unetgrad.h, 64 x 64 latent, random weights):
`hedit_unet_forward`, `hedit_unet_forward_keep` and `hedit_unet_backward`, warm, measured with device events around `--reps`
back-to-back calls, with the gradient workspace; then the attention-backward kernels alone (csrc/attnbwd.hip) at the 64 x 64
level's shape (N = 4096, 8 heads, d = 40).  One JSON line per measurement.

    python tools/unet_grad_time.py [--batches 1 2] [--reps 5] [--tiny]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib  # noqa: E402
from hedit.unet import SD15_CONFIG, TINY_CONFIG, UNet2DConditionModel  # noqa: E402


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the small test configuration (a quick check of the tool itself)")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = TINY_CONFIG if a.tiny else SD15_CONFIG
    model = UNet2DConditionModel(cfg, device=dev, grad=True)
    model.init_random(0)
    lib, h = model._lib, model._h
    S, D = cfg["sample_size"], cfg["cross_attention_dim"]
    g = torch.Generator().manual_seed(0)
    for B in a.batches:
        x = torch.randn(B, 4, S, S, generator=g).to(dev)
        u = torch.randn(B, 4, S, S, generator=g).to(dev)
        ctx = torch.randn(B, 77, D, generator=g).to(dev)
        eps, dx = torch.empty_like(x), torch.empty_like(x)
        need = lib.hedit_unet_grad_workspace_bytes(h, B, S, S)
        assert need > 0, lib.hedit_last_error().decode()
        ws = torch.empty(max(need, lib.hedit_unet_workspace_bytes(h, B, S, S)), dtype=torch.uint8, device=dev)

        def fwd():
            _lib.check(lib.hedit_unet_forward(h, _lib.ptr(x), 501.0, _lib.ptr(ctx), B, S, S, None, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))

        def keep():
            _lib.check(lib.hedit_unet_forward_keep(h, _lib.ptr(x), 501.0, _lib.ptr(ctx), B, S, S, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))

        def bwd():
            _lib.check(lib.hedit_unet_backward(h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None))

        for f in (fwd, keep, bwd):
            f()
        torch.cuda.synchronize()
        ms_f, ms_k = timed(fwd, a.reps), timed(keep, a.reps)
        ms_b = timed(bwd, a.reps)           # on the last kept forward
        lib.hedit_unet_release(h)
        print(json.dumps({"B": B, "S": S, "reps": a.reps, "forward_ms": round(ms_f, 3), "forward_keep_ms": round(ms_k, 3),
                          "backward_ms": round(ms_b, 3), "backward_over_forward": round(ms_b / ms_f, 3),
                          "grad_workspace_GiB": round(need / 2 ** 30, 3), "finite": bool(torch.isfinite(dx).all())}), flush=True)
        del ws
    # the attention-backward kernels alone, at the 64 x 64 level of SD-1.5
    Bn, heads, N, d = 1, 8, 4096, 40
    C = heads * d
    dt = _lib.storage_dtype()
    qk = (torch.randn(Bn * N, 2 * C, generator=g) * 0.3).to(dev, dt)
    v, o, do = ((torch.randn(Bn * N, C, generator=g)).to(dev, dt) for _ in range(3))
    dq, dk, dv = (torch.empty(Bn * N, C, dtype=dt, device=dev) for _ in range(3))
    st = torch.empty(lib.hedit_k_attn_bwd_ws_bytes(Bn, N, heads), dtype=torch.uint8, device=dev)
    kctx, vctx = ((torch.randn(Bn * 80, C, generator=g)).to(dev, dt) for _ in range(2))
    qkp = qk.data_ptr()

    def self_bwd():
        _lib.check(lib.hedit_k_attn_bwd(qkp, 2 * C, qkp + 2 * C, 2 * C, _lib.ptr(v), C, _lib.ptr(o), C, _lib.ptr(do), C, _lib.ptr(dq), C,
                                        _lib.ptr(dk), _lib.ptr(dv), Bn, N, heads, d, _lib.ptr(st), None))

    def cross_bwd():
        _lib.check(lib.hedit_k_cross_attn_bwd_q(qkp, 2 * C, _lib.ptr(kctx), C, _lib.ptr(vctx), C, _lib.ptr(o), C, _lib.ptr(do), C,
                                                _lib.ptr(dq), C, Bn, N, heads, d, None))

    for f in (self_bwd, cross_bwd):
        f()
    torch.cuda.synchronize()
    ms_s, ms_c = timed(self_bwd, a.reps), timed(cross_bwd, a.reps)
    flops = 10.0 * Bn * heads * N * N * d * (6.0 / 5.0)      # five products, S recomputed once more by the second kernel
    print(json.dumps({"attn_bwd": {"B": Bn, "heads": heads, "N": N, "d": d}, "self_ms": round(ms_s, 3), "cross_q_ms": round(ms_c, 3),
                      "self_TFLOPs_executed": round(flops / ms_s / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
