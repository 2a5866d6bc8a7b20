"""CPU tests of hedit.image_prep: Pillow's fixed-point resample restated (the tap tables the device kernel is fed, plus a numpy
two-pass restatement) against the installed PIL byte for byte, the two normalisation look-up tables against the host formulas
they stand for, the two size-and-crop conventions, and the ABI bookkeeping of the new entries."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import imgprep_ref as IR  # noqa: E402
from hedit import image_prep as IP  # noqa: E402
from hedit.clip_score import CLIP_MEAN, CLIP_STD, preprocess_pil  # noqa: E402


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
@pytest.mark.parametrize("sizes", IR.RESIZES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_the_restated_resample_is_pils(sizes, filter):
    (w, h), (ow, oh) = sizes
    a = IR.image(h, w, 7 * w + h)
    want = IR.pil_resize(a, ow, oh, filter)
    got = IP.resize_host(a, ow, oh, filter)
    assert got.shape == want.shape == (oh, ow, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())


def test_tables():
    assert IP.resample_table(16, 16, "bilinear") is None and IP.resample_table(16, 16, "bicubic") is None
    taps, bounds = IP.resample_table(512, 224, "bilinear")
    assert taps.shape == (224, 7) and taps.dtype == np.int32 and bounds.shape == (224, 2)        # support 512 / 224 -> ceil 3 -> 7 taps
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 512).all() and (bounds[:, 1] <= 7).all()
    assert (np.abs(taps.sum(1) - (1 << 22)) <= 4).all()                                            # normalised before the rounding
    for i, (f, c) in enumerate(bounds):
        assert (taps[i, c:] == 0).all()
    taps, _ = IP.resample_table(512, 224, "bicubic")
    assert taps.shape == (224, 11) and (taps < 0).any()
    taps, bounds = IP.resample_table(20, 24, "bicubic")                                             # upscale: the filter keeps its support
    assert taps.shape == (24, 5)
    with pytest.raises(ValueError):
        IP.resample_table(0, 4, "bilinear")
    with pytest.raises(KeyError):
        IP.resample_table(8, 4, "lanczos")


def test_the_transformers_path_is_preprocess_pil():
    a = IR.image(56, 40, 3)                                              # 40 wide, 56 high
    want = preprocess_pil(a, 16)
    got = IR.prep_host(a, 16, "transformers")
    assert got.dtype == np.float32 and got.shape == (3, 16, 16) and np.array_equal(got, want)
    b = IR.image(40, 57, 4)                                              # landscape, an odd margin
    assert np.array_equal(IR.prep_host(b, 16, "transformers"), preprocess_pil(Image.fromarray(b), 16))


def test_the_torchvision_path_is_its_restatement():
    for h, w, seed in ((56, 40, 5), (40, 57, 6), (23, 16, 7)):
        a = IR.image(h, w, seed)
        got = IR.prep_host(a, 16, "torchvision")
        want = IR.torchvision_ref(a, 16)
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy()), (h, w)


def test_look_up_tables():
    lt, lv = IP.norm_lut("transformers"), IP.norm_lut("torchvision")
    assert lt.shape == lv.shape == (3, 256) and lt.dtype == lv.dtype == np.float32
    v = torch.arange(256, dtype=torch.uint8)
    mean, std = torch.tensor(CLIP_MEAN)[:, None], torch.tensor(CLIP_STD)[:, None]
    assert np.array_equal(lv, ((v.float() / 255)[None] - mean).div(std).numpy())                   # ToTensor, Normalize: fp32 throughout
    x = (np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32)
    assert np.array_equal(lt, (x[None] - np.array(CLIP_MEAN, np.float32)[:, None]) / np.array(CLIP_STD, np.float32)[:, None])
    # on the 256 uint8 values the two rescales round to the same fp32: the tables are kept apart because the formulas are
    assert np.array_equal(lt, lv)
    with pytest.raises(ValueError):
        IP.norm_lut("other")


def test_sizes_and_crops():
    assert IP.resized_size(512, 512, 224) == (224, 224)
    assert IP.resized_size(40, 56, 16) == (16, 22) and IP.resized_size(56, 40, 16) == (22, 16)
    assert IP.resized_size(37, 53, 16) == (16, int(16 * 53 / 37))
    # odd margins: 21 -> margin 5, 5 // 2 = 2, round(2.5) = 2 (to even); 23 -> margin 7, 7 // 2 = 3, round(3.5) = 4
    assert IP.crop_offset(21, 16, "floor") == 2 and IP.crop_offset(21, 16, "round") == 2
    assert IP.crop_offset(23, 16, "floor") == 3 and IP.crop_offset(23, 16, "round") == 4
    assert IP.crop_offset(19, 16, "floor") == 1 and IP.crop_offset(19, 16, "round") == 2         # 1.5 -> 2
    assert IP.crop_offset(224, 224, "floor") == IP.crop_offset(224, 224, "round") == 0
    for n in range(16, 40):
        assert 0 <= IP.crop_offset(n, 16, "round") <= n - 16 and IP.crop_offset(n, 16, "floor") == (n - 16) // 2
    with pytest.raises(ValueError):
        IP.crop_offset(20, 16, "ceil")
    # the conventions pair the filter with the crop rule
    assert IP.CONVENTIONS == {"transformers": ("bicubic", "floor"), "torchvision": ("bilinear", "round")}


def test_host_refusals():
    p = IP.NativeImagePrep()                                             # nothing touches the GPU before the host checks
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.resize_crop(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4, 4, "bilinear", 0, 0, 4, 4, "torchvision")
    with pytest.raises(RuntimeError, match="no CPU path"):
        IP.NativeImagePrep("cpu")([IR.image(8, 8, 1)], 4, "torchvision")
    with pytest.raises(ValueError, match="one size"):
        p([IR.image(8, 8, 1), IR.image(8, 9, 1)], 4, "torchvision")
    with pytest.raises(ValueError, match="convention"):
        p([IR.image(8, 8, 1)], 4, "pil")
    with pytest.raises(ValueError, match="uint8"):
        IP.image_u8(np.zeros((4, 4, 3), dtype=np.float32))


def test_new_exports_are_declared():
    from hedit import _lib
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    want = {"hedit_image_prep", "hedit_image_prep_workspace_bytes", "hedit_clip_direction"}
    declared = set(re.findall(r"\b(hedit_(?:image_prep|clip_direction)[a-z0-9_]*)\s*\(", hdr))
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith(("hedit_image_prep", "hedit_clip_direction"))}
    assert IP.MAX_BATCH == int(re.search(r"#define HEDIT_IMAGE_PREP_MAX_BATCH (\d+)", hdr).group(1)) == 64
    assert IP.MAX_TAPS == int(re.search(r"#define HEDIT_IMAGE_PREP_MAX_TAPS (\d+)", hdr).group(1))
    from hedit import local_clip_score as LC
    assert LC.MAX_PAIRS == int(re.search(r"#define HEDIT_CLIP_DIRECTION_MAX_PAIRS (\d+)", hdr).group(1)) == 64
    assert LC.MAX_TEMPLATES == int(re.search(r"#define HEDIT_CLIP_DIRECTION_MAX_TEMPLATES (\d+)", hdr).group(1)) == 256
    assert os.path.exists(_lib.LIB_PATH), "build libhedit_hip.so first: python h-edit_amd/build.py"
    for path in (_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), "libhedit_hip_f16.so")):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, n) for n in want), path
    ws = _lib.lib().hedit_image_prep_workspace_bytes
    assert ws(1, 512, 224) == 512 * 224 * 3 and ws(3, 20, 16) == 3 * 20 * 16 * 3
    assert ws(0, 8, 8) == 0 and ws(65, 8, 8) == 0 and ws(1, 0, 8) == 0 and ws(1, 8, 16385) == 0
