#!/usr/bin/env python3
"""Generate tests/golden/g21_face_ef.npz by RUNNING THE REFERENCE's Edit Friendly face loop
(face-swapping/inversion/ef.py, UNMODIFIED) on the reference's pixel UNet (diffusion/diffusion.py::Model) at toy size,
in the pattern of make_golden.py::gen_face_child: its own interpreter with face-swapping/ on sys.path, FACE_TINY,
face_state_dict, the TinyIdLoss / TinyLpips stand-ins, and the SDE inversion (zs, xts) and mask recorded in g11_face.npz.
Needs the reference tree, like make_golden.py; the output is data only.

    python tests/golden/make_golden_face_ef.py

Cases (T = 10, eta = 1, weight_edit_face = 100, the reference default).  Only late starts: with these toy weights the
10-step chain is chaotic from skip 0 .. 4 (the no-edit run alone moves by 1.2 relative under bf16 autocast), so a full-
length comparison would pin nothing."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FACE_TINY, REF_FACE, face_state_dict, npy  # noqa: E402

# name, skip, identity, LPIPS, mask
CASES = (("ef_s6", 6, True, True, False), ("ef_s6_idmask", 6, True, False, True), ("ef_s6_lp", 6, False, True, False),
         ("ef_s7_mask", 7, True, True, True), ("ef_s8", 8, True, True, False))


def main():
    if not os.path.isdir(REF_FACE):
        raise SystemExit("reference tree not present")
    torch.set_num_threads(4)
    torch.set_grad_enabled(True)
    sys.path.insert(0, REF_FACE)
    import warnings
    warnings.filterwarnings("ignore")
    from diffusion.diffusion import Model
    from diffusion.diffusion_utils import get_beta_schedule
    import inversion.ef as ef_mod
    ef_mod.tqdm = lambda x, *a, **k: x
    from helpers.tiny import TinyIdLoss, TinyLpips
    model = Model(dict(FACE_TINY)).eval()
    model.load_state_dict(face_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    for p_ in model.parameters():
        p_.requires_grad_(False)
    g11 = np.load(os.path.join(HERE, "g11_face.npz"))
    zs, xts, mask = torch.from_numpy(g11["zs"]), torch.from_numpy(g11["xts"]), torch.from_numpy(g11["mask"])
    betas = torch.from_numpy(get_beta_schedule(beta_schedule="linear", beta_start=0.0001, beta_end=0.02,
                                               num_diffusion_timesteps=1000)).float()
    T = 10
    seq = (np.arange(0, 1000, 1000 // T) + 1)[::-1]
    idl, lp = TinyIdLoss(), TinyLpips()
    d = {}
    for name, skip, use_id, use_lp, use_mask in CASES:
        after = T - skip
        out = ef_mod.ef(model, lp if use_lp else None, idl if use_id else None, xts[after].clone(), betas, seq, eta=1.0,
                        zs=zs[:after], weight_edit_face=100.0, after_skip_steps=after, num_inference_steps=T,
                        soft_face_mask=mask if use_mask else None)
        d[name] = npy(out)
    np.savez_compressed(os.path.join(HERE, "g21_face_ef.npz"), **d)
    print("g21_face_ef.npz", os.path.getsize(os.path.join(HERE, "g21_face_ef.npz")), "bytes")


if __name__ == "__main__":
    main()
