"""The pixel metrics of the evaluator restated in numpy: fp32 ``a = u8 / 255`` (times the mask) and ``d = a - b``, fp64 for
everything after that, SSIM over the (H - 10) x (W - 10) x 3 windows that lie inside the image (what the evaluator's
reflect-pad-then-crop computes), the separable 11-tap Gaussian applied rows first, taps in rising order -- the arithmetic
csrc/pixmetrics.hip documents.  Also the shapes and the seeded inputs the CPU and GPU tests share; every reference is
computed once per process and handed out read-only.
"""
import functools

import numpy as np

from hedit.pixel_score import GAUSS_TAPS

C1, C2 = 1e-4, 9e-4
SHAPES = ((11, 11), (12, 43), (64, 64), (75, 53))      # one window; ragged + odd W (unaligned rows); aligned; ragged over several tiles
BIG = (512, 512)                                       # the workload's own size
KINDS = ("noise", "smooth", "onebit", "same")
# torch fp32 path (MetricsCalculator("cpu")) vs this restatement, worst over SHAPES + BIG x KINDS x parts as first measured:
# mse 1.4e-7 relative, psnr 5.9e-6 dB, ssim 1.4e-5 absolute; the tests allow 4 x that (another host's conv kernels)
GAP_MSE_REL, GAP_PSNR_DB, GAP_SSIM = 4 * 1.4e-7, 4 * 5.9e-6, 4 * 1.4e-5


def _blur_valid(z):
    """z fp64 (H, W, 3) -> (H - 10, W - 10, 3): rows first (along W), then columns, each a sum over taps 0 ... 10 from 0.0"""
    H, W, _ = z.shape
    rows = np.zeros((H, W - 10, 3))
    for k, w in enumerate(GAUSS_TAPS):
        rows = rows + w * z[:, k:k + W - 10]
    out = np.zeros((H - 10, W - 10, 3))
    for k, w in enumerate(GAUSS_TAPS):
        out = out + w * rows[k:k + H - 10]
    return out


def part_metrics(a8, b8, ma=None, mb=None):
    """(mse, psnr, ssim) of one pair; ma / mb: H x W arrays of 0 / 1 multiplied onto the images, or None"""
    a = a8.astype(np.float32) / np.float32(255.0)
    b = b8.astype(np.float32) / np.float32(255.0)
    if ma is not None:
        a = a * ma.astype(np.float32)[:, :, None]
    if mb is not None:
        b = b * mb.astype(np.float32)[:, :, None]
    assert a.dtype == np.float32 and b.dtype == np.float32
    d = (a - b).astype(np.float64)
    mse = float((d * d).sum() / d.size)
    psnr = float("inf") if mse == 0.0 else float(10.0 * np.log10(1.0 / mse))
    x, y = a.astype(np.float64), b.astype(np.float64)
    mu_a, mu_b, saa, sbb, sab = (_blur_valid(z) for z in (x, y, x * x, y * y, x * y))
    va, vb, vab = saa - mu_a * mu_a, sbb - mu_b * mu_b, sab - mu_a * mu_b
    q = ((2.0 * (mu_a * mu_b) + C1) * (2.0 * vab + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (va + vb + C2))
    return mse, psnr, float(q.sum() / q.size)


def metrics(a8, b8, mask_pred=None, mask_gt=None):
    """3 x 3 float64: parts (whole, edit, unedit) x (mse, psnr, ssim), a missing mask = all ones, NaN rows without any mask --
    the layout and the rules of hedit_pixel_metrics"""
    out = np.full((3, 3), np.nan)
    out[0] = part_metrics(a8, b8)
    if mask_pred is not None or mask_gt is not None:
        ones = np.ones(a8.shape[:2], dtype=np.uint8)
        ma, mb = ones if mask_pred is None else mask_pred, ones if mask_gt is None else mask_gt
        out[1] = part_metrics(a8, b8, ma, mb)
        out[2] = part_metrics(a8, b8, 1 - ma, 1 - mb)
    return out


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pair(H, W, kind):
    """seeded uint8 H x W x 3 pairs: uniform noise; a smooth pattern plus noise; a pair differing in one bit of one pixel;
    an identical pair"""
    rng = np.random.default_rng(1000 * H + W + 7 * KINDS.index(kind))
    if kind == "noise":
        a, b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([127.5 + 100.0 * np.sin(0.11 * xx + 0.07 * yy + c) * np.cos(0.05 * yy - 0.03 * xx * c) for c in range(3)], axis=2)
        a = np.clip(base + rng.normal(0.0, 6.0, base.shape), 0, 255).astype(np.uint8)
        if kind == "smooth":
            b = np.clip(base + rng.normal(0.0, 6.0, base.shape), 0, 255).astype(np.uint8)
        else:
            b = a.copy()
            if kind == "onebit":
                b[H // 2, W // 3, 1] ^= 4
    return _ro(a), _ro(b)


@functools.lru_cache(maxsize=None)
def rect_mask(H, W):
    """a rectangular 0 / 1 mask (uint8 H x W) off the tile grid, touching neither all nor none of the image"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[H // 4:H // 4 + max(1, H // 2), W // 5:W // 5 + max(1, (2 * W) // 3)] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def expected(H, W, kind, masks="both"):
    """the restatement for pair(H, W, kind) with masks "both" / "pred" / "gt" / "none" of rect_mask(H, W)"""
    a, b = pair(H, W, kind)
    m = rect_mask(H, W)
    return _ro(metrics(a, b, m if masks in ("both", "pred") else None, m if masks in ("both", "gt") else None))
