"""Child process of tests/test_gpu_clip_score.py: the toy image towers of tests/golden/g20_clipimg.* in the storage build
named by HEDIT_STORAGE (one format per process, hedit/_lib.py), embeddings written to the .npz given as argv[1].

    HEDIT_STORAGE=f16 python tests/helpers/clipimg_child.py out.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "h-edit_amd")):
    sys.path.insert(0, p)

from helpers import clipimg_ref as CR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.clip_score import NativeClipImage  # noqa: E402


def embeddings(device="cuda:0"):
    """name -> fp32 array: three images through each toy tower in one call"""
    import torch
    out = {}
    for tag, cfg, seed in (("e17", CR.TOY17, 501), ("e257", CR.TOY257, 502)):
        enc = NativeClipImage.from_clip_state_dict(CR.clipimg_weights(**cfg), device=device)
        out[tag] = enc(CR.test_images(3, cfg["input_resolution"], seed)).cpu().numpy()
        torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    d = embeddings()
    d["is_f16"] = np.array([_lib.lib().hedit_storage_is_f16()])
    np.savez(sys.argv[1], **d)
