"""Test infrastructure for hedit.image_prep / csrc/imgprep.hip: reproducible uint8 images, the installed PIL as the reference
of the resample, the host composition of a whole convention from the module's own tables, and torchvision's preprocessing
(Resize on a PIL image, CenterCrop, ToTensor, Normalize) restated with PIL and torch.  Nothing here is product code."""
import numpy as np
import torch
from PIL import Image

from hedit import image_prep as IP
from hedit.clip_score import CLIP_MEAN, CLIP_STD

# ((width, height), (new width, new height)): the big downscale of the evaluator, odd sizes, an upscale, one pass only, no pass
RESIZES = (((512, 512), (224, 224)), ((37, 53), (16, 22)), ((20, 31), (24, 37)), ((64, 48), (16, 12)), ((33, 33), (16, 16)),
           ((50, 80), (16, 25)), ((16, 16), (16, 16)))
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def image(h, w, seed):
    """uint8 (h, w, 3): smooth ramps, noise and saturated blocks, so that taps of both signs meet 0 and 255"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([xx / max(w - 1, 1), yy / max(h - 1, 1), (xx + yy) / max(w + h - 2, 1)], -1)
    a = 0.5 * base + 0.5 * rng.random((h, w, 3))
    a[: h // 3, : w // 3] = rng.integers(0, 2, (h // 3, w // 3, 3))     # hard 0 / 255 edges: bicubic overshoot gets clamped
    return np.clip(a * 255.0, 0, 255).astype(np.uint8)


def pil_resize(a, ow, oh, filter):
    return np.array(Image.fromarray(a).resize((ow, oh), resample=PIL_FILTER[filter]))


def geometry(h, w, size, convention):
    """(new width, new height, top, left) of a convention"""
    _, rule = IP.CONVENTIONS[convention]
    nw, nh = IP.resized_size(w, h, size)
    return nw, nh, IP.crop_offset(nh, size, rule), IP.crop_offset(nw, size, rule)


def prep_host(a, size, convention):
    """float32 (3, size, size): the module's tables, crop rule and look-up table composed on the host"""
    filter, _ = IP.CONVENTIONS[convention]
    nw, nh, top, left = geometry(a.shape[0], a.shape[1], size, convention)
    r = IP.resize_host(a, nw, nh, filter)[top:top + size, left:left + size]
    lut = IP.norm_lut(convention)
    return np.stack([lut[c][r[:, :, c]] for c in range(3)])


def torchvision_ref(a, size):
    """torchvision's Compose([Resize(size), CenterCrop(size), ToTensor(), Normalize(mean, std)]) on a PIL image, restated:
    PIL bilinear to (size, int(size * long / short)), crop offsets int(round((n - size) / 2.0)), uint8 -> fp32 / 255, then
    (x - mean) / std in fp32 through torch"""
    img = Image.fromarray(a)
    w, h = img.size
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    img = img.resize((nw, nh), Image.BILINEAR)
    top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
    x = torch.from_numpy(np.array(img)[top:top + size, left:left + size]).permute(2, 0, 1).contiguous()
    x = x.to(torch.float32).div(255)
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(CLIP_STD, dtype=torch.float32)[:, None, None]
    return (x - mean) / std
