#!/usr/bin/env python3
"""Device time of the SD UNet's context-gradient pass at the SD-1.5 shape (csrc/unetgrad.h, 64 x 64 latent, random weights):
`hedit_unet_forward_keep` + `hedit_unet_backward` (the yardstick) against `hedit_unet_forward_keep` + `hedit_unet_backward_ctx`,
with and without d_x, warm, measured with device events around `--reps` back-to-back calls, with the gradient workspace of the
two kinds of handle; then, per level of SD-1.5 (N = 4096 / 1024 / 256 / 64 queries, 8 heads, d = 40 / 80 / 160 / 160), the
cross-attention backward's two halves alone: `hedit_k_cross_attn_bwd_q` (the dq kernel) and `hedit_k_cross_attn_bwd_kv` (the dq
kernel's statistics sweep + the partial kernel + the reduce kernel).  One JSON line per measurement.  For the share of the
partial kernel, the reduce kernel and the final GEMM inside a backward, run `--trace B` under a kernel trace in a run of its
own: it does one warm-up and `--reps` backward_ctx calls and nothing else.

    python tools/ctx_grad_time.py [--batches 1 8] [--reps 5] [--tiny] [--trace B]
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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the small test configuration (a quick check of the tool itself)")
    ap.add_argument("--trace", type=int, default=0, metavar="B", help="only one warm-up and --reps backward_ctx calls at batch B")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = TINY_CONFIG if a.tiny else SD15_CONFIG
    model = UNet2DConditionModel(cfg, device=dev, grad="context")
    model.init_random(0)
    lib, h = model._lib, model._h
    S, D = cfg["sample_size"], cfg["cross_attention_dim"]
    g = torch.Generator().manual_seed(0)
    for B in ([a.trace] if a.trace else a.batches):
        x = torch.randn(B, 4, S, S, generator=g).to(dev)
        u = torch.randn(B, 4, S, S, generator=g).to(dev)
        ctx = torch.randn(B, 77, D, generator=g).to(dev)
        eps, dx, dc = torch.empty_like(x), torch.empty_like(x), torch.empty_like(ctx)
        need = lib.hedit_unet_grad_workspace_bytes(h, B, S, S)
        assert need > 0, lib.hedit_last_error().decode()
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def keep():
            _lib.check(lib.hedit_unet_forward_keep(h, _lib.ptr(x), 501.0, _lib.ptr(ctx), B, S, S, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))

        def bwd():
            _lib.check(lib.hedit_unet_backward(h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None))

        def bwd_ctx():
            _lib.check(lib.hedit_unet_backward_ctx(h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(dc), _lib.ptr(ws), None))

        def bwd_ctx_only():
            _lib.check(lib.hedit_unet_backward_ctx(h, _lib.ptr(u), None, _lib.ptr(dc), _lib.ptr(ws), None))

        if a.trace:
            keep()
            bwd_ctx()
            torch.cuda.synchronize()
            ms = timed(bwd_ctx, a.reps)
            print(json.dumps({"trace": True, "B": B, "reps": a.reps, "backward_ctx_ms": round(ms, 3)}), flush=True)
            lib.hedit_unet_release(h)
            return
        for f in (keep, bwd, bwd_ctx, bwd_ctx_only):
            f()
        torch.cuda.synchronize()
        ms_k = timed(keep, a.reps)
        ms_b, ms_c, ms_o = timed(bwd, a.reps), timed(bwd_ctx, a.reps), timed(bwd_ctx_only, a.reps)      # on the last kept forward
        lib.hedit_unet_release(h)
        print(json.dumps({"B": B, "S": S, "reps": a.reps, "forward_keep_ms": round(ms_k, 3), "backward_ms": round(ms_b, 3),
                          "backward_ctx_ms": round(ms_c, 3), "backward_ctx_no_dx_ms": round(ms_o, 3),
                          "keep_plus_backward_ms": round(ms_k + ms_b, 3), "keep_plus_backward_ctx_ms": round(ms_k + ms_c, 3),
                          "ctx_over_plain": round((ms_k + ms_c) / (ms_k + ms_b), 4), "grad_workspace_GiB": round(need / 2 ** 30, 3),
                          "finite": bool(torch.isfinite(dx).all() and torch.isfinite(dc).all())}), flush=True)
        del ws
    if a.tiny:
        return
    # the two halves of the cross-attention backward alone, at the four levels of SD-1.5
    dt = _lib.storage_dtype()
    for Bn in a.batches:
        for N, d in ((4096, 40), (1024, 80), (256, 160), (64, 160)):
            heads = 8
            C = heads * d
            q = (torch.randn(Bn * N, C, generator=g) * 0.3).to(dev, dt)
            o, do = ((torch.randn(Bn * N, C, generator=g)).to(dev, dt) for _ in range(2))
            kctx, vctx = ((torch.randn(Bn * 80, C, generator=g)).to(dev, dt) for _ in range(2))
            dq = torch.empty(Bn * N, C, dtype=dt, device=dev)
            dk, dv = (torch.empty(Bn * 80, C, dtype=dt, device=dev) for _ in range(2))
            ws = torch.empty(lib.hedit_k_cross_attn_bwd_kv_ws_bytes(Bn, N, heads, d), dtype=torch.uint8, device=dev)

            def cross_q():
                _lib.check(lib.hedit_k_cross_attn_bwd_q(_lib.ptr(q), C, _lib.ptr(kctx), C, _lib.ptr(vctx), C, _lib.ptr(o), C, _lib.ptr(do), C,
                                                        _lib.ptr(dq), C, Bn, N, heads, d, None))

            def cross_kv():
                _lib.check(lib.hedit_k_cross_attn_bwd_kv(_lib.ptr(q), C, _lib.ptr(kctx), C, _lib.ptr(vctx), C, _lib.ptr(o), C, _lib.ptr(do), C,
                                                         _lib.ptr(dk), _lib.ptr(dv), C, Bn, N, heads, d, _lib.ptr(ws), None))

            for f in (cross_q, cross_kv):
                f()
            torch.cuda.synchronize()
            ms_q, ms_kv = timed(cross_q, 4 * a.reps), timed(cross_kv, 4 * a.reps)
            print(json.dumps({"cross_attn_bwd": {"B": Bn, "heads": heads, "N": N, "d": d}, "dq_ms": round(ms_q, 4),
                              "stats_partial_reduce_ms": round(ms_kv, 4), "blocks": Bn * heads * ((N + 127) // 128)}), flush=True)


if __name__ == "__main__":
    main()
