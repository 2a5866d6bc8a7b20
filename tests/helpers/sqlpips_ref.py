"""PARITY UNPINNED.  A torch restatement of SqueezeNet-LPIPS -- torchmetrics' LearnedPerceptualImagePatchSimilarity(
net_type='squeeze'), what the reference's text-guided/evaluation/matrics_calculator.py:276,329-347 scores with -- for the
tests of csrc/sqlpips.hip / hedit/lpips_score.py.  torchvision, lpips and torchmetrics are not installed here and the
reference tree holds no vector for this metric: nothing pins this file to the packages.  What it restates is their
published network:

  ScalingLayer (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450)
  torchvision squeezenet1_1.features: 0 Conv 3->64 k3 stride 2 no padding, 1 ReLU (tap 0: 64), 2 MaxPool k3 s2 ceil_mode,
  3 4 Fire (tap 1: 128), 5 MaxPool, 6 7 Fire (tap 2: 256), 8 MaxPool, 9 Fire (tap 3: 384), 10 Fire (tap 4: 384),
  11 Fire (tap 5: 512), 12 Fire (tap 6: 512);  Fire: x = relu(squeeze1x1(x)), cat[relu(expand1x1(x)), relu(expand3x3(x, pad 1))]
  distance = sum_k mean_hw sum_c lin_k[c] (a^_c - b^_c)^2, a^ = tap / (channel L2 norm + 1e-10)

It runs in fp64 (the reference of the GPU tests) or fp32, on any device, on the parameters of hedit.lpips_score.SqueezeLpipsNet.
"""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
FIRE_IDX = (3, 4, 6, 7, 9, 10, 11, 12)
TAP_AFTER = {4: 1, 7: 2, 9: 3, 10: 4, 11: 5, 12: 6}        # features index -> tap
POOL_BEFORE = (3, 6, 9)                                   # features 2, 5, 8 are the pools


def taps(params, x, dtype=torch.float64):
    """x (N, 3, H, W) in [-1, 1] -> the seven tap tensors (N, C_k, H_k, W_k)"""
    p = {k: v.to(device=x.device, dtype=dtype) for k, v in params.items()}
    x = x.to(dtype)
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(device=x.device, dtype=dtype)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=torch.float32).to(device=x.device, dtype=dtype)[None, :, None, None]
    x = (x - shift) / scale
    x = F.relu(F.conv2d(x, p["features.0.weight"], p["features.0.bias"], stride=2))
    out = [x]
    for i in FIRE_IDX:
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, kernel_size=3, stride=2, ceil_mode=True)
        pre = f"features.{i}."
        s = F.relu(F.conv2d(x, p[pre + "squeeze.weight"], p[pre + "squeeze.bias"]))
        x = torch.cat([F.relu(F.conv2d(s, p[pre + "expand1x1.weight"], p[pre + "expand1x1.bias"])),
                       F.relu(F.conv2d(s, p[pre + "expand3x3.weight"], p[pre + "expand3x3.bias"], padding=1))], dim=1)
        if i in TAP_AFTER:
            out.append(x)
    return out


def distance(params, a, b, dtype=torch.float64):
    """(N,) LPIPS(a_n, b_n) in `dtype`"""
    with torch.no_grad():
        ta, tb = taps(params, a, dtype), taps(params, b, dtype)
        total = 0
        for k, (fa, fb) in enumerate(zip(ta, tb)):
            na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            lin = params[f"lin{k}.model.1.weight"].to(device=a.device, dtype=dtype)
            total = total + F.conv2d((na - nb) ** 2, lin).mean(dim=(1, 2, 3))
    return total


def uint8_pair(H, W, seed):
    """a = random uint8 image, b = clip(a + 0.1 randn) back in uint8: two (H, W, 3) arrays"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.float64) / 255 + 0.1 * rng.standard_normal((H, W, 3)), 0, 1)
    return a, np.uint8(np.round(b * 255))


def upper_half_mask(H, W):
    """(H, W, 3) float mask, 0 on the upper half"""
    m = np.ones((H, W, 3))
    m[:H // 2] = 0
    return m
