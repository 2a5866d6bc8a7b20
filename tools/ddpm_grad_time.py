#!/usr/bin/env python3
"""Device time of the pixel UNet's input-gradient pass at CelebA-HQ shape (csrc/ddpm.hip, random weights): `hedit_ddpm_forward`,
`hedit_ddpm_forward_keep` and `hedit_ddpm_backward`, warm, measured with device events around `--reps` back-to-back calls;
then Edit Friendly faces/s for `--faces` faces in lock-step at `--steps` steps with the reward networks of
`main_edit_face.py --mode ef --random_init` (IR-SE50 identity reward, LPIPS-VGG; random weights).  One JSON line per measurement.

    python tools/ddpm_grad_time.py [--batches 1 8] [--reps 5] [--faces 8] [--steps 100] [--no-ef]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib  # noqa: E402
from hedit.diffusion import Model  # noqa: E402


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
    ap.add_argument("--faces", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-ef", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    model = Model(device=dev, grad=True)
    model.init_random(0)
    lib, h = model._lib, model._h
    S = model.resolution
    g = torch.Generator().manual_seed(0)
    for B in a.batches:
        x = torch.randn(B, 3, S, S, generator=g).to(dev)
        u = torch.randn(B, 3, S, S, generator=g).to(dev)
        eps, dx = torch.empty_like(x), torch.empty_like(x)
        need = lib.hedit_ddpm_grad_workspace_bytes(h, B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def fwd():
            _lib.check(lib.hedit_ddpm_forward(h, _lib.ptr(x), 501.0, B, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))

        def keep():
            _lib.check(lib.hedit_ddpm_forward_keep(h, _lib.ptr(x), 501.0, B, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))

        def bwd():
            _lib.check(lib.hedit_ddpm_backward(h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None))

        for f in (fwd, keep, bwd):
            f()
        torch.cuda.synchronize()
        ms_f, ms_k = timed(fwd, a.reps), timed(keep, a.reps)
        ms_b = timed(bwd, a.reps)           # on the last kept forward
        lib.hedit_ddpm_release(h)
        print(json.dumps({"B": B, "S": S, "reps": a.reps, "forward_ms": round(ms_f, 3), "forward_keep_ms": round(ms_k, 3),
                          "backward_ms": round(ms_b, 3), "backward_over_forward": round(ms_b / ms_f, 3),
                          "grad_workspace_GiB": round(need / 2 ** 30, 3)}), flush=True)
        del ws
    if a.no_ef:
        return
    from hedit.arcface import IDLoss
    from hedit.arcface.lpips_loss import LPIPS_Loss
    from hedit.inversion.ef_face import ef
    n, T = a.faces, a.steps
    betas = torch.from_numpy(np.linspace(0.0001, 0.02, 1000, dtype=np.float64)).float().to(dev)
    seq = (np.arange(0, 1000, 1000 // T) + 1)[::-1]
    refs = (torch.rand(n, 3, S, S, generator=g) * 2 - 1).to(dev)
    srcs = (torch.rand(n, 3, S, S, generator=g) * 2 - 1).to(dev)
    idloss = IDLoss(ref=refs, weights=None, device=dev, seed=0)
    lpipsloss = LPIPS_Loss(src=srcs, weights=None, device=dev, seed=0)
    xT = torch.randn(n, 3, S, S, generator=g).to(dev)
    zs = torch.randn(T, n, 3, S, S, generator=g).to(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    out = ef(model, lpipsloss, idloss, xT, betas, seq, eta=1.0, zs=zs, weight_edit_face=100.0, after_skip_steps=T,
             num_inference_steps=T, per_image=True)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(json.dumps({"ef_faces": n, "steps": T, "seconds": round(dt, 3), "faces_per_s": round(n / dt, 4),
                      "finite": bool(torch.isfinite(out).all())}), flush=True)


if __name__ == "__main__":
    main()
