"""Image preprocessing of the CLIP metrics on the native executor (``hedit_image_prep`` of libhedit_hip.so, csrc/imgprep.hip):
PIL's ``Image.resize`` on 8-bit RGB, a centre crop, ``/ 255`` and CLIP's mean / std, bit for bit what the host code does.

The kernel knows no filter.  This module builds, in float64 and exactly as Pillow's ``Resample.c`` does for 8-bit images, the
fixed-point tap table of one axis (``resample_table``), the two normalisation look-up tables (``norm_lut``) and the two
size-and-crop conventions:

  transformers  (``CLIPImageProcessor``, what ``hedit.clip_score.preprocess_pil`` restates): bicubic, crop offset
                ``(n - size) // 2``, ``f32(f64(v) * (1 / 255))``, then fp32 mean and std
  torchvision   (``Resize(size)`` on a PIL image, ``CenterCrop``, ``ToTensor``, ``Normalize``: the preprocessing of the
                reference's local_clip metric, local_clip_evaluation.py:62-68): bilinear, crop offset
                ``int(round((n - size) / 2.0))``, fp32 ``v / 255``, then fp32 mean and std

Both resize the shortest edge to ``size`` and the long edge to ``int(size * long / short)``.  ``resize_host`` is the numpy
restatement of the two passes (the tests compare it, and the kernel, with the installed PIL byte for byte).  There is no CPU
path of the device call.
"""
import math

import numpy as np
import torch

from .clip_score import CLIP_MEAN, CLIP_STD
from .native import NativeOwner

MAX_BATCH = 64            # HEDIT_IMAGE_PREP_MAX_BATCH of include/hedit.h
MAX_TAPS = 1024           # HEDIT_IMAGE_PREP_MAX_TAPS
MAX_SIDE = 16384
PRECISION_BITS = 22       # Resample.c: 32 - 8 - 2
_NO_CPU = "NativeImagePrep runs on the HIP executor only (there is no CPU path)"


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}
# the two conventions: (filter, crop rule)
CONVENTIONS = {"transformers": ("bicubic", "floor"), "torchvision": ("bilinear", "round")}


def resample_table(in_size, out_size, filter):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis -> (taps int32 [out][ksize], bounds int32 [out][2] =
    (first source index, count)); None when the size does not change (Pillow skips the pass)."""
    fn, fsupport = FILTERS[filter]
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_table: sizes {in_size} -> {out_size}")
    if in_size == out_size:
        return None
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    taps = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), in_size)
        w = [fn((x + first - center + 0.5) / fs) for x in range(last - first)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        taps[i, :len(w)] = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
        bounds[i] = (first, len(w))
    return taps, bounds


def _pass_host(a, table, axis):
    """one pass of Resample.c along `axis` of a uint8 (H, W, 3) array"""
    if table is None:
        return a
    taps, bounds = table
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((len(taps),) + a.shape[1:], dtype=np.uint8)
    for i, (first, count) in enumerate(bounds):
        acc = np.tensordot(taps[i, :count].astype(np.int64), a[first:first + count], axes=1) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_host(a, out_w, out_h, filter):
    """``np.array(Image.fromarray(a).resize((out_w, out_h), filter))`` restated: horizontal pass, uint8, vertical pass"""
    a = np.asarray(a)
    h, w = a.shape[:2]
    return _pass_host(_pass_host(a, resample_table(w, out_w, filter), 1), resample_table(h, out_h, filter), 0)


def resized_size(w, h, size):
    """(new width, new height): the shortest edge to `size`, the long edge ``int(size * long / short)`` -- transformers'
    get_resize_output_image_size and torchvision's Resize(int) alike"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(size), int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def crop_offset(n, size, rule):
    """the first index of a centre crop of `size` out of `n`: ``floor`` = (n - size) // 2 (transformers), ``round`` =
    int(round((n - size) / 2.0)) with Python's rounding (torchvision's center_crop)"""
    if rule == "floor":
        return (n - size) // 2
    if rule == "round":
        return int(round((n - size) / 2.0))
    raise ValueError(f"crop rule {rule!r}: floor or round")


def norm_lut(convention):
    """float32 [3][256]: what the convention's rescale + normalise make of every uint8 value, per channel"""
    v = np.arange(256)
    if convention == "transformers":
        x = (v.astype(np.float64) * (1 / 255)).astype(np.float32)
    elif convention == "torchvision":
        x = v.astype(np.float32) / np.float32(255)
    else:
        raise ValueError(f"convention {convention!r}: one of {', '.join(CONVENTIONS)}")
    mean = np.array(CLIP_MEAN, dtype=np.float32)[:, None]
    std = np.array(CLIP_STD, dtype=np.float32)[:, None]
    return np.ascontiguousarray((x[None, :] - mean) / std)


def image_u8(img):
    """a PIL image or an array -> the contiguous uint8 H x W x 3 array the kernel reads"""
    if hasattr(img, "convert"):
        img = img.convert("RGB")
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"image prep: expected a PIL image or a uint8 (H, W, 3) array, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


class NativeImagePrep(NativeOwner):
    """``resize_crop`` is one native call on a device uint8 batch; ``__call__`` takes what the evaluator holds.  Tables are
    built and uploaded once per (in size, out size, filter) and per convention."""
    batch_invariant = True

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.calls = 0                # native calls made (tests count them)
        self._tables = {}             # (in, out, filter) -> None or (taps, bounds, ksize, host bounds)
        self._luts = {}

    def _table(self, n_in, n_out, filter):
        key = (int(n_in), int(n_out), filter)
        if key not in self._tables:
            t = resample_table(n_in, n_out, filter)
            if t is not None:
                if t[0].shape[1] > MAX_TAPS:
                    raise ValueError(f"image prep: {n_in} -> {n_out} ({filter}) needs {t[0].shape[1]} taps per pixel, the kernel takes {MAX_TAPS}")
                t = (torch.from_numpy(t[0]).to(self.device), torch.from_numpy(t[1]).to(self.device), t[0].shape[1], t[1])
            self._tables[key] = t
        return self._tables[key]

    def _lut(self, lut):
        if isinstance(lut, str):
            if lut not in self._luts:
                self._luts[lut] = torch.from_numpy(norm_lut(lut)).to(self.device)
            return self._luts[lut]
        if not torch.is_tensor(lut) or lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256):
            raise ValueError("image prep: a look-up table is a convention's name or a float32 (3, 256) tensor")
        return lut.to(self.device).contiguous()

    def resize_crop(self, src, out_w, out_h, filter, top, left, crop_h, crop_w, lut, return_u8=False):
        """src: CUDA uint8 (B, H, W, 3) -> CUDA float32 (B, 3, crop_h, crop_w): the window [top, top + crop_h) x
        [left, left + crop_w) of the images resized to out_w x out_h, through `lut`.  With ``return_u8`` also the window's
        pixels, uint8 (B, crop_h, crop_w, 3).  ONE native call."""
        from . import _lib
        if self.device.type != "cuda" or not torch.is_tensor(src) or not src.is_cuda:
            raise RuntimeError(_NO_CPU + ": pass a CUDA tensor")
        if src.dim() != 4 or src.shape[3] != 3 or src.dtype != torch.uint8:
            raise ValueError(f"image prep: expected a uint8 (B, H, W, 3) tensor, got {src.dtype} {tuple(src.shape)}")
        B, H, W, _ = src.shape
        if B < 1 or B > MAX_BATCH:
            raise ValueError(f"image prep: batch {B} outside [1, {MAX_BATCH}]")
        for v in (H, W, out_w, out_h):
            if v < 1 or v > MAX_SIDE:
                raise ValueError(f"image prep: side {v} outside [1, {MAX_SIDE}]")
        if crop_h < 1 or crop_w < 1 or top < 0 or left < 0 or top + crop_h > out_h or left + crop_w > out_w:
            raise ValueError(f"image prep: the crop ({top}, {left}, {crop_h}, {crop_w}) leaves the resized image ({out_h} x {out_w})")
        dev = self.device
        tx, ty = self._table(W, out_w, filter), self._table(H, out_h, filter)
        if ty is None:
            row0, nrows = top, crop_h
        else:
            b = ty[3][top:top + crop_h]
            row0 = int(b[:, 0].min())
            nrows = int((b[:, 0] + b[:, 1]).max()) - row0
        table = self._lut(lut)
        src = src.to(dev).contiguous()
        out = torch.empty(B, 3, crop_h, crop_w, device=dev, dtype=torch.float32)
        u8 = torch.empty(B, crop_h, crop_w, 3, device=dev, dtype=torch.uint8) if return_u8 else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            need = lib.hedit_image_prep_workspace_bytes(B, nrows, crop_w)
            self._grow("_ws", max(need, 1), dev)
            _lib.check(lib.hedit_image_prep(_lib.ptr(src), B, H, W, out_h, out_w, top, left, crop_h, crop_w,
                                            _lib.ptr(tx and tx[0]), _lib.ptr(tx and tx[1]), tx[2] if tx else 0,
                                            _lib.ptr(ty and ty[0]), _lib.ptr(ty and ty[1]), ty[2] if ty else 0, row0, nrows,
                                            _lib.ptr(table), _lib.ptr(out), _lib.ptr(u8), _lib.ptr(self._ws), self._ws.numel(), _lib.cur_stream()))
        self.calls += 1
        return (out, u8) if return_u8 else out

    def __call__(self, images, size, convention):
        """A list of equal-sized PIL images / uint8 (H, W, 3) arrays -> CUDA float32 (B, 3, size, size) under `convention`
        (``transformers`` or ``torchvision``): one upload and one native call per MAX_BATCH images."""
        if convention not in CONVENTIONS:
            raise ValueError(f"convention {convention!r}: one of {', '.join(CONVENTIONS)}")
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        arrays = [image_u8(im) for im in images]
        if not arrays:
            raise ValueError("image prep: no images")
        if len({a.shape for a in arrays}) != 1:
            raise ValueError("image prep: the images of one call must have one size")
        filter, rule = CONVENTIONS[convention]
        h, w = arrays[0].shape[:2]
        size = int(size)
        nw, nh = resized_size(w, h, size)
        top, left = crop_offset(nh, size, rule), crop_offset(nw, size, rule)
        outs = []
        for i in range(0, len(arrays), MAX_BATCH):
            src = torch.from_numpy(np.stack(arrays[i:i + MAX_BATCH])).to(self.device)
            outs.append(self.resize_crop(src, nw, nh, filter, top, left, size, size, convention))
        return outs[0] if len(outs) == 1 else torch.cat(outs)
