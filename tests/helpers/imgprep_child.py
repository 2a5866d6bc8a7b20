"""Child process of tests/test_gpu_image_prep.py and tests/test_gpu_local_clip.py: the image preprocessing and the direction
head in the storage build named by HEDIT_STORAGE (one format per process, hedit/_lib.py), results written to the .npz given as
argv[1].

    HEDIT_STORAGE=f16 python tests/helpers/imgprep_child.py out.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "h-edit_amd")):
    sys.path.insert(0, p)

from helpers import imgprep_ref as IR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.image_prep import NativeImagePrep  # noqa: E402
from hedit.local_clip_score import direction  # noqa: E402


def head_inputs(P, T, E, seed):
    """fp32 (P, 2, T, E) and (P, 2, E), a function of the arguments alone"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, 2, T, E)).astype(np.float32), rng.standard_normal((P, 2, E)).astype(np.float32)


def results(device="cuda:0"):
    """name -> array: both conventions on three 40 x 56 images, a two-pass uint8 case, and the head at (5, 3, 64)"""
    import torch
    prep = NativeImagePrep(device)
    imgs = [IR.image(56, 40, 90 + i) for i in range(3)]
    out = {c: prep(imgs, 16, c).cpu().numpy() for c in ("transformers", "torchvision")}
    src = torch.from_numpy(np.stack([IR.image(53, 37, 95)])).to(device)
    out["u8"] = prep.resize_crop(src, 16, 22, "bicubic", 0, 0, 22, 16, "torchvision", return_u8=True)[1].cpu().numpy()
    txt, img = head_inputs(5, 3, 64, 96)
    out["head"] = direction(torch.from_numpy(txt).to(device), torch.from_numpy(img).to(device)).cpu().numpy()
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    d = results()
    d["is_f16"] = np.array([_lib.lib().hedit_storage_is_f16()])
    np.savez(sys.argv[1], **d)
