"""Child process of tests/test_gpu_sqlpips.py: SqueezeNet-LPIPS distances of fixed pairs in the storage build named by
HEDIT_STORAGE (one format per process, hedit/_lib.py), written to the .npz given as argv[1].

    HEDIT_STORAGE=f16 python tests/helpers/sqlpips_child.py out.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "h-edit_amd")):
    sys.path.insert(0, p)

from helpers import sqlpips_ref as SR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.lpips_score import NativeSqueezeLpips, preprocess_pair  # noqa: E402

SEED = 11
CASES = ((36, 52, 3), (64, 64, 2))          # (H, W, pairs)


def pairs(H, W, n, seed0=300):
    """n preprocessed pairs of H x W, the odd ones with the upper half masked: two (n, 3, H, W) tensors"""
    import torch
    out = []
    for i in range(n):
        a8, b8 = SR.uint8_pair(H, W, seed0 + 7 * i + H)
        m = SR.upper_half_mask(H, W) if i % 2 else None
        out.append(preprocess_pair(a8, b8, m, m))
    return torch.stack([p[0] for p in out]), torch.stack([p[1] for p in out])


def distances(device="cuda:0"):
    """name -> fp32 array: every case in one native call"""
    import torch
    m = NativeSqueezeLpips(device=device, seed=SEED)
    out = {}
    for H, W, n in CASES:
        a, b = pairs(H, W, n)
        out[f"d{H}x{W}"] = m.distance(a.to(device), b.to(device)).cpu().numpy()
        torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    d = distances()
    d["is_f16"] = np.array([_lib.lib().hedit_storage_is_f16()])
    np.savez(sys.argv[1], **d)
