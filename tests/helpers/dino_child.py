"""Child process of tests/test_gpu_dino.py: DINO keys and structure distances of fixed inputs in the storage build named by
HEDIT_STORAGE (one format per process, hedit/_lib.py), written to the .npz given as argv[1].

    HEDIT_STORAGE=f16 python tests/helpers/dino_child.py out.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "h-edit_amd")):
    sys.path.insert(0, p)

from helpers import dino_ref as DR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.dino_score import NativeDinoStructure  # noqa: E402

CASES = (("t145", 3), ("t785", 2))          # (parity case, pairs)


def pairs(name, n, seed0=300):
    """n pairs of the case's input size, float32 in 0...255, the odd ones with the upper half masked: two (n, 3, S, S) tensors"""
    import torch
    S = DR.CASES[name][5]
    m = DR.upper_half_mask(S).astype(np.float32)
    A, B = [], []
    for i in range(n):
        a8, b8 = DR.uint8_pair(S, seed0 + 7 * i + S)
        a, b = a8.astype(np.float32), b8.astype(np.float32)
        if i % 2:
            a, b = a * m, b * m
        A.append(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))))
        B.append(torch.from_numpy(np.ascontiguousarray(b.transpose(2, 0, 1))))
    return torch.stack(A), torch.stack(B)


def results(device="cuda:0"):
    """name -> fp32 array: per case the distances of its pairs (one native call) and the keys of its first two images"""
    import torch
    out = {}
    for name, n in CASES:
        m = NativeDinoStructure(DR.net_of(name), device=device)
        a, b = pairs(name, n)
        out[f"d_{name}"] = m.distance(a.to(device), b.to(device)).cpu().numpy()
        out[f"k_{name}"] = m.keys(a[:2].to(device)).cpu().numpy()
        torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    d = results()
    d["is_f16"] = np.array([_lib.lib().hedit_storage_is_f16()])
    np.savez(sys.argv[1], **d)
