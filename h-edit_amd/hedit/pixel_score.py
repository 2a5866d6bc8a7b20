"""The pixel metrics of the PIE-Bench evaluator on the native executor (``hedit_pixel_metrics`` of libhedit_hip.so,
csrc/pixmetrics.hip): the ``mse*`` / ``psnr*`` / ``ssim*`` columns -- torchmetrics' MeanSquaredError,
PeakSignalNoiseRatio(data_range=1) and StructuralSimilarityIndexMeasure(data_range=1) of the reference's
text-guided/evaluation/matrics_calculator.py:272-279, by the formulas evaluation/evaluation.py states for the torch path.

One native call takes up to ``MAX_BATCH`` uint8 pairs with their 0 / 1 masks and returns, per pair, parts (whole, edit,
unedit) x metrics (mse, psnr, ssim) as float64: ``a = float(u8) / 255`` times the mask and ``d = a - b`` in fp32, everything
after that in fp64.  There are no weights, no CPU path, no gradients, and masks are binary: a mask with
other values is refused (the torch path of ``MetricsCalculator`` takes any mask).
"""
import numpy as np
import torch

from .native import NativeOwner

MAX_BATCH = 64            # HEDIT_PIXEL_METRICS_MAX_BATCH of include/hedit.h
MIN_SIDE = 11             # one 11 x 11 SSIM window
METRICS = ("mse", "psnr", "ssim")     # the columns of a 3 x 3 result; its rows are the parts whole, edit, unedit
# the 1-D taps behind the evaluator's _gauss(11, 1.5): exp(-(d / 1.5) ** 2 / 2) / sum in fp32 (PM_TAPS of csrc/pixmetrics.hip)
GAUSS_TAPS = tuple(float.fromhex(h) for h in ("0x1.0d957p-10", "0x1.f1fdf8p-8", "0x1.26eb18p-5", "0x1.bff0fcp-4", "0x1.b43c3ep-3", "0x1.10656p-2",
                                              "0x1.b43c3ep-3", "0x1.bff0fcp-4", "0x1.26eb18p-5", "0x1.f1fdf8p-8", "0x1.0d957p-10"))
_NO_CPU = "NativePixelMetrics runs on the HIP executor only (there is no CPU path)"


def image_u8(img):
    """a PIL image or an array -> the uint8 H x W x 3 array the kernel reads"""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"pixel metrics: expected a uint8 H x W x 3 image, got {a.dtype} {a.shape}")
    if a.shape[0] < MIN_SIDE or a.shape[1] < MIN_SIDE:
        raise ValueError(f"pixel metrics: images of {a.shape[0]} x {a.shape[1]}, SSIM's window needs at least {MIN_SIDE} x {MIN_SIDE}")
    return np.ascontiguousarray(a)


def mask_u8(mask, H, W):
    """an H x W or H x W x 3 mask of zeros and ones (any dtype) -> uint8 H x W; None stays None"""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.ndim == 3:
        if m.shape[2] not in (1, 3) or not (m == m[:, :, :1]).all():
            raise ValueError(f"pixel metrics: a mask of shape {m.shape} that is not channel-identical; the native path takes one mask per pixel "
                             "(the torch path, MetricsCalculator without pixel=, takes any mask)")
        m = m[:, :, 0]
    if m.shape != (H, W):
        raise ValueError(f"pixel metrics: a mask of shape {m.shape} for images of {H} x {W}")
    if not ((m == 0) | (m == 1)).all():
        raise ValueError("pixel metrics: mask values other than 0 and 1; the native path takes binary masks only "
                         "(the torch path, MetricsCalculator without pixel=, takes any mask)")
    return np.ascontiguousarray(m.astype(np.uint8))


class NativePixelMetrics(NativeOwner):
    """``metrics`` is one native call; ``scores`` / ``score`` take what the evaluator holds.  Results are bit-identical whatever
    the batch (``batch_invariant``), and equal images give exactly mse 0, psnr +inf and ssim 1."""
    batch_invariant = True

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.calls = 0                # native calls made (tests count them)

    def metrics(self, pred, gt, mask_pred=None, mask_gt=None):
        """pred, gt: CUDA uint8 (N, H, W, 3); mask_pred, mask_gt: CUDA uint8 (N, H, W) of 0 / 1, or None = all ones ->
        CUDA float64 (N, 3, 3) = parts (whole, edit, unedit) x (mse, psnr, ssim); with both masks None the edit and unedit rows
        are NaN.  ONE native call."""
        from . import _lib
        for t in (pred, gt, mask_pred, mask_gt):
            if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
                raise RuntimeError(_NO_CPU + ": pass CUDA tensors")
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        if pred.dim() != 4 or pred.shape[3] != 3 or pred.shape != gt.shape or pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
            raise ValueError(f"metrics: expected two uint8 (N, H, W, 3) tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        N, H, W, _ = pred.shape
        if N < 1 or N > MAX_BATCH:
            raise ValueError(f"metrics: batch {N} outside [1, {MAX_BATCH}]")
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"metrics: images of {H} x {W}, SSIM's window needs at least {MIN_SIDE} x {MIN_SIDE}")
        for m in (mask_pred, mask_gt):
            if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != (N, H, W)):
                raise ValueError(f"metrics: a mask must be uint8 {(N, H, W)}, got {m.dtype} {tuple(m.shape)}")
        dev = self.device
        pred, gt = pred.to(dev).contiguous(), gt.to(dev).contiguous()
        mask_pred = None if mask_pred is None else mask_pred.to(dev).contiguous()
        mask_gt = None if mask_gt is None else mask_gt.to(dev).contiguous()
        out = torch.empty(N, 3, 3, device=dev, dtype=torch.float64)
        lib = _lib.lib()
        with torch.cuda.device(dev):
            need = lib.hedit_pixel_metrics_workspace_bytes(N, H, W)
            self._grow("_ws", max(need, 8), dev)
            _lib.check(lib.hedit_pixel_metrics(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(mask_pred), _lib.ptr(mask_gt), N, H, W, _lib.ptr(out),
                                               _lib.ptr(self._ws), self._ws.numel(), _lib.cur_stream()))
        self.calls += 1
        return out

    def scores(self, items):
        """[(img_pred, img_gt[, mask_pred[, mask_gt]]), ...] of one image size -> one 3 x 3 float64 array per item, parts
        (whole, edit, unedit) x (mse, psnr, ssim); ONE native call per MAX_BATCH pairs.  A missing mask is all ones; an item
        without any mask has NaN edit and unedit rows whatever it is grouped with."""
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        prepared = []
        for it in items:
            it = tuple(it) + (None,) * (4 - len(it))
            a, b = image_u8(it[0]), image_u8(it[1])
            if a.shape != b.shape:
                raise ValueError(f"pixel metrics: image shapes should be the same, got {a.shape} and {b.shape}")
            prepared.append((a, b, mask_u8(it[2], *a.shape[:2]), mask_u8(it[3], *a.shape[:2])))
        if not prepared:
            return []
        if len({p[0].shape for p in prepared}) != 1:
            raise ValueError("scores: the pairs of one call must have one image size")
        H, W = prepared[0][0].shape[:2]
        ones = None
        out = []
        for i in range(0, len(prepared), MAX_BATCH):
            chunk = prepared[i:i + MAX_BATCH]
            masks = []
            for k in (2, 3):
                if all(p[k] is None for p in chunk):
                    masks.append(None)
                    continue
                ones = np.ones((H, W), dtype=np.uint8) if ones is None else ones
                masks.append(torch.from_numpy(np.stack([ones if p[k] is None else p[k] for p in chunk])).to(self.device))
            pred = torch.from_numpy(np.stack([p[0] for p in chunk])).to(self.device)
            gt = torch.from_numpy(np.stack([p[1] for p in chunk])).to(self.device)
            res = self.metrics(pred, gt, masks[0], masks[1]).cpu().numpy()
            for p, r in zip(chunk, res):
                if p[2] is None and p[3] is None:
                    r[1:] = np.nan
                out.append(r)
        return out

    def score(self, metric, img_pred, img_gt, mask_pred=None, mask_gt=None):
        """one metric of one pair: the edit part (image times its mask) when a mask is given, else the whole image"""
        if metric not in METRICS:
            raise ValueError(f"pixel metrics: unknown metric {metric!r} (one of {', '.join(METRICS)})")
        r = self.scores([(img_pred, img_gt, mask_pred, mask_gt)])[0]
        return float(r[0 if mask_pred is None and mask_gt is None else 1, METRICS.index(metric)])
