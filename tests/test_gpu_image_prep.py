"""-m gpu: the native image preprocessing (hedit_image_prep of csrc/imgprep.hip, behind hedit.image_prep.NativeImagePrep)
against the installed PIL and the host formulas.  Everything here is integer arithmetic and a table look-up, so every
comparison is bit for bit: the uint8 pixels against ``Image.resize``, the fp32 tensor against ``preprocess_pil`` and against
torchvision's preprocessing restated (tests/helpers/imgprep_ref.py), a batch against its single calls, one storage build
against the other."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers import imgprep_ref as IR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit import image_prep as IP  # noqa: E402
from hedit.clip_score import NativeClip, preprocess_pil  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
# ((width, height), (new width, new height), filters): odd sizes both ways, an upscale, one pass only (the height stays), the
# other pass only, no pass at all, and the evaluator's 512 -> 224
U8_CASES = ((((37, 53), (16, 22)), ("bilinear", "bicubic")), (((20, 31), (24, 37)), ("bilinear", "bicubic")),
            (((50, 80), (16, 80)), ("bilinear", "bicubic")), (((50, 80), (50, 25)), ("bicubic",)), (((16, 16), (16, 16)), ("bilinear", "bicubic")),
            (((512, 512), (224, 224)), ("bilinear",)))


@pytest.fixture(scope="module")
def prep():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return IP.NativeImagePrep(G.dev())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.dev())


@pytest.mark.parametrize("case", U8_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0][0] + c[0][1]))
def test_pixels_are_pils(prep, case):
    ((w, h), (ow, oh)), filters = case
    a = IR.image(h, w, 3 * w + h)
    for filter in filters:
        want = IR.pil_resize(a, ow, oh, filter)
        out, u8 = prep.resize_crop(_dev(a[None]), ow, oh, filter, 0, 0, oh, ow, "torchvision", return_u8=True)
        G.sync()
        got = u8[0].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (filter, int((got != want).sum()))
        lut = IP.norm_lut("torchvision")
        assert np.array_equal(out[0].cpu().numpy(), np.stack([lut[c][want[:, :, c]] for c in range(3)]))
        # a window alone: only the crop is computed, with the same bits
        ch, cw = max(oh // 2, 1), max(ow // 3, 1)
        top, left = (oh - ch) // 2, ow - cw
        _, part = prep.resize_crop(_dev(a[None]), ow, oh, filter, top, left, ch, cw, "torchvision", return_u8=True)
        G.sync()
        assert np.array_equal(part[0].cpu().numpy(), want[top:top + ch, left:left + cw]), filter


def test_the_fp32_tensor_is_the_hosts(prep):
    for h, w, seed in ((56, 40, 3), (40, 57, 4), (23, 16, 5), (16, 16, 6)):
        a = IR.image(h, w, seed)
        got = prep([a], 16, "transformers")
        want = torch.from_numpy(preprocess_pil(a, 16))
        G.sync()
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 3, 16, 16)
        assert torch.equal(got[0].cpu(), want), ("transformers", h, w)
        assert torch.equal(prep([a], 16, "torchvision")[0].cpu(), IR.torchvision_ref(a, 16)), ("torchvision", h, w)


def test_pixel_values_of_the_clip_wrapper(prep):
    """NativeClip.pixel_values(native=True): the host path's tensor, images of several sizes and a preprocessed tensor mixed in"""
    import types
    clip = NativeClip(types.SimpleNamespace(embed_dim=32, device=G.dev(), input_resolution=16), types.SimpleNamespace(proj_dim=32), None)
    from PIL import Image
    ready = torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(1))
    images = [IR.image(56, 40, 11), Image.fromarray(IR.image(40, 57, 12)), ready, IR.image(56, 40, 13)]
    host = clip.pixel_values(images)
    assert not host.is_cuda                                              # the default is the host path, unchanged
    dev = clip.pixel_values(images, native=True)
    G.sync()
    assert dev.is_cuda and torch.equal(dev.cpu(), host)
    clip.native_preprocess = True
    assert torch.equal(clip.pixel_values(images).cpu(), host)


def test_batch_invariance_bit_for_bit(prep):
    imgs = [IR.image(53, 37, 20 + i) for i in range(3)]
    for conv in ("transformers", "torchvision"):
        n = prep.calls
        a = prep(imgs, 16, conv)
        assert prep.calls == n + 1                                       # one native call for the whole list
        singles = torch.cat([prep([im], 16, conv) for im in imgs])
        G.sync()
        assert torch.equal(a, singles) and torch.equal(a, prep(imgs, 16, conv))
        assert not torch.equal(a[0], a[1])


def test_errors_are_reported_before_anything_is_launched(prep):
    lib = _lib.lib()
    H, W, Hr, Wr = 53, 37, 22, 16
    src = _dev(IR.image(H, W, 1)[None].repeat(2, 0))
    tx, ty = prep._table(W, Wr, "bilinear"), prep._table(H, Hr, "bilinear")
    lut = prep._lut("torchvision")
    out = torch.full((2, 3, Hr, Wr), -7.0, device=G.dev())
    need = lib.hedit_image_prep_workspace_bytes(2, H, Wr)
    ws = torch.empty(need, dtype=torch.uint8, device=G.dev())
    base = dict(src=src, B=2, H=H, W=W, Hr=Hr, Wr=Wr, top=0, left=0, ch=Hr, cw=Wr, tx=tx[0], bx=tx[1], kx=tx[2], ty=ty[0], by=ty[1], ky=ty[2],
                row0=0, nrows=H, lut=lut, out=out, ws=ws, nbytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return lib.hedit_image_prep(_lib.ptr(a["src"]), a["B"], a["H"], a["W"], a["Hr"], a["Wr"], a["top"], a["left"], a["ch"], a["cw"],
                                    _lib.ptr(a["tx"]), _lib.ptr(a["bx"]), a["kx"], _lib.ptr(a["ty"]), _lib.ptr(a["by"]), a["ky"], a["row0"],
                                    a["nrows"], _lib.ptr(a["lut"]), _lib.ptr(a["out"]), None, _lib.ptr(a["ws"]), a["nbytes"], _lib.cur_stream())

    bad = ((dict(src=None), "null"), (dict(lut=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
           (dict(B=0), "1 <= B <= 64"), (dict(B=65), "1 <= B <= 64"), (dict(H=0), "[1, 16384]"), (dict(W=16385), "[1, 16384]"),
           (dict(Hr=0), "resized"), (dict(Wr=16385), "resized"),
           (dict(top=1), "crop leaves"), (dict(left=-1), "crop leaves"), (dict(cw=Wr + 1), "crop leaves"), (dict(ch=0), "crop leaves"),
           (dict(kx=0), "taps per output index"), (dict(ky=IP.MAX_TAPS + 1), "taps per output index"),
           (dict(tx=None, bx=None), "unchanged width"), (dict(ty=None, by=None), "unchanged height"), (dict(bx=None), "go together"),
           (dict(row0=1), "source rows"), (dict(nrows=0), "source rows"),
           (dict(nbytes=need - 1), "workspace too small"))
    for kw, msg in bad:
        rc = call(**kw)
        err = lib.hedit_last_error().decode()
        assert rc == -1 and "bad argument" in err and "image_prep" in err and msg in err, (kw, rc, err)
    G.sync()
    assert (out == -7.0).all()                                           # nothing ran
    assert call() == 0
    G.sync()
    want = IR.pil_resize(IR.image(H, W, 1), Wr, Hr, "bilinear")
    table = IP.norm_lut("torchvision")
    assert np.array_equal(out[1].cpu().numpy(), np.stack([table[c][want[:, :, c]] for c in range(3)]))
    # the wrapper refuses on the host what the entry would
    with pytest.raises(ValueError, match="leaves the resized image"):
        prep.resize_crop(src, Wr, Hr, "bilinear", 0, 1, Hr, Wr, "torchvision")
    with pytest.raises(ValueError, match="batch 65"):
        prep.resize_crop(torch.zeros(65, 4, 4, 3, dtype=torch.uint8, device=G.dev()), 4, 4, "bilinear", 0, 0, 4, 4, "torchvision")
    with pytest.raises(ValueError, match="taps per pixel"):
        prep.resize_crop(torch.zeros(1, 2, 600, 3, dtype=torch.uint8, device=G.dev()), 1, 2, "bicubic", 0, 0, 2, 1, "torchvision")


def test_the_other_storage_build_gives_the_same_bits(tmp_path):
    """ONE child process in the other storage format (bf16 parent -> libhedit_hip_f16.so, and the reverse): nothing in
    csrc/imgprep.hip reads the 16-bit type -- the preprocessing and the direction head alike"""
    from helpers import imgprep_child as CH
    other = "bf16" if _lib.STORAGE == "f16" else "f16"
    out = tmp_path / "child.npz"
    env = dict(os.environ, HEDIT_STORAGE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "imgprep_child.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    c = np.load(out)
    assert int(c["is_f16"][0]) == (1 if other == "f16" else 0)
    mine = CH.results()
    for k, v in mine.items():
        assert np.array_equal(v, c[k], equal_nan=True), k
    assert np.isfinite(mine["head"]).all() and np.array_equal(mine["u8"][0], IR.pil_resize(IR.image(53, 37, 95), 16, 22, "bicubic"))
