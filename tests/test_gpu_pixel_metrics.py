"""-m gpu: the native pixel metrics (hedit_pixel_metrics of csrc/pixmetrics.hip) through the C ABI, against the fp64 numpy
restatement tests/helpers/pixel_ref.py (computed once per process on the CPU) and against the evaluator's torch code.

Limits against the restatement, from the arithmetic (the fp32 values a, b, d are the same on both sides):
  mse   1e-9 relative: d * d is exact in fp64; at most 786 432 terms are summed at 2^-53 each
  psnr  1e-8 dB
  ssim  1e-10 absolute: everything is fp64, the worst amplification is the division by c2
Equal images: exactly 0.0 / +inf / 1.0.  Against MetricsCalculator("cpu"): 4 x the gap measured between that code and the
restatement (pixel_ref.GAP_*).  Batch and repeat comparisons are bit for bit.

MEASURED (MI355X, both storage builds; every comparison prints its figures with -s before it asserts), worst over all shapes,
inputs and mask combinations: against the restatement mse 3.1e-16 relative, psnr 1.8e-15 dB, ssim 5.6e-16 (512 x 512: 2.0e-16 /
0 / 5.6e-16); against the torch path on the CPU mse 1.5e-7, psnr 3.2e-6 dB, ssim 1.2e-5.  The file takes 3 s inside pytest.
"""
import csv
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers import pixel_ref as PR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.pixel_score import NativePixelMetrics  # noqa: E402

MODES = ("both", "pred", "gt", "none")


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(G.dev())


def native(a, b, mp=None, mg=None):
    """uint8 arrays (N, H, W, 3) and (N, H, W) or None -> float64 (N, 3, 3), one hedit_pixel_metrics call"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib.lib()
    N, H, W, _ = a.shape
    ta, tb, tmp, tmg = _dev(a), _dev(b), _dev(mp), _dev(mg)
    out = torch.empty(N, 3, 3, dtype=torch.float64, device=G.dev())
    ws = torch.empty(lib.hedit_pixel_metrics_workspace_bytes(N, H, W), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_pixel_metrics(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(tmp), _lib.ptr(tmg), N, H, W, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                       _lib.cur_stream()))
    G.sync()
    return out.cpu().numpy()


def _kinds(H, W, mode):
    """the four input kinds of one shape as one batch, with the rectangular mask on the sides `mode` names"""
    a = np.stack([PR.pair(H, W, k)[0] for k in PR.KINDS])
    b = np.stack([PR.pair(H, W, k)[1] for k in PR.KINDS])
    m = np.stack([PR.rect_mask(H, W)] * len(PR.KINDS))
    return a, b, (m if mode in ("both", "pred") else None), (m if mode in ("both", "gt") else None)


def _check_against_restatement(got, ref, what):
    """got, ref: (3, 3).  NaN rows must be NaN rows; an exact 0 / inf / 1 of the restatement must be exact here"""
    worst = [0.0, 0.0, 0.0]
    for p in range(3):
        if np.isnan(ref[p]).all():
            assert np.isnan(got[p]).all(), (what, p, got[p])
            continue
        mse, psnr, ssim = ref[p]
        if mse == 0.0:
            assert got[p, 0] == 0.0 and np.isposinf(got[p, 1]) and got[p, 2] == 1.0, (what, p, got[p])
            continue
        e = (abs(got[p, 0] - mse) / mse, abs(got[p, 1] - psnr), abs(got[p, 2] - ssim))
        worst = [max(w, x) for w, x in zip(worst, e)]
    print(f"[pixel parity] {what}: mse {worst[0]:.2e} relative, psnr {worst[1]:.2e} dB, ssim {worst[2]:.2e}")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-8 and worst[2] <= 1e-10, (what, worst, got, ref)


@pytest.mark.parametrize("shape", PR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_the_fp64_restatement(shape):
    H, W = shape
    for mode in MODES:
        got = native(*_kinds(H, W, mode))
        for k, kind in enumerate(PR.KINDS):
            _check_against_restatement(got[k], PR.expected(H, W, kind, mode), f"{H} x {W} {kind} masks={mode}")
        if mode == "none":
            assert np.isnan(got[:, 1:]).all() and np.isfinite(got[:, 0, 0]).all()
    same = PR.KINDS.index("same")
    got = native(*_kinds(H, W, "both"))[same]
    assert (got[:, 0] == 0.0).all() and np.isposinf(got[:, 1]).all() and (got[:, 2] == 1.0).all()


def test_the_workloads_own_size():
    """512 x 512, one case, N = 1: against the restatement and against the torch path"""
    from evaluation import evaluation as EV
    H, W = PR.BIG
    a, b = PR.pair(H, W, "smooth")
    m = PR.rect_mask(H, W)
    got = native(a[None], b[None], m[None], m[None])[0]
    _check_against_restatement(got, PR.expected(H, W, "smooth"), "512 x 512 smooth masks=both")
    mc = EV.MetricsCalculator("cpu")
    m3 = m[:, :, None].repeat(3, axis=2).astype(np.float64)
    _check_against_torch(mc, got, a, b, m3, "512 x 512 smooth")


def _check_against_torch(mc, got, a, b, m3, what):
    worst = [0.0, 0.0, 0.0]
    for p, (ma, mb) in enumerate(((None, None), (m3, m3), (1 - m3, 1 - m3))):
        t = (mc.calculate_mse(a, b, ma, mb), mc.calculate_psnr(a, b, ma, mb), mc.calculate_ssim(a, b, ma, mb))
        e = (abs(got[p, 0] - t[0]) / t[0] if t[0] else abs(got[p, 0]), 0.0 if got[p, 1] == t[1] else abs(got[p, 1] - t[1]), abs(got[p, 2] - t[2]))
        worst = [max(w, x) for w, x in zip(worst, e)]
    print(f"[pixel native vs torch] {what}: mse {worst[0]:.2e} relative, psnr {worst[1]:.2e} dB, ssim {worst[2]:.2e}")
    assert worst[0] <= PR.GAP_MSE_REL and worst[1] <= PR.GAP_PSNR_DB and worst[2] <= PR.GAP_SSIM, (what, worst)


@pytest.mark.parametrize("shape", PR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_the_torch_path(shape):
    """ties the native numbers to the code users run today"""
    from evaluation import evaluation as EV
    H, W = shape
    mc = EV.MetricsCalculator("cpu")
    m3 = PR.rect_mask(H, W)[:, :, None].repeat(3, axis=2).astype(np.float64)
    got = native(*_kinds(H, W, "both"))
    for k, kind in enumerate(PR.KINDS):
        _check_against_torch(mc, got[k], *PR.pair(H, W, kind), m3, f"{H} x {W} {kind}")


def test_batch_and_repeat_invariance():
    H, W = 75, 53
    a, b, _, _ = _kinds(H, W, "none")
    a, b = np.concatenate([a, b[:1]]), np.concatenate([b, a[:1]])                  # five distinct pairs
    m = np.stack([np.roll(PR.rect_mask(H, W), 3 * i, axis=1) for i in range(5)])
    assert len({x.tobytes() for x in a}) == 5 and len({x.tobytes() for x in m}) == 5
    batch = native(a, b, m, m)
    again = native(a, b, m, m)
    assert batch.tobytes() == again.tobytes()
    for n in range(5):
        alone = native(a[n:n + 1], b[n:n + 1], m[n:n + 1], m[n:n + 1])
        assert alone.tobytes() == batch[n:n + 1].tobytes(), n
    assert np.isfinite(batch[:, :, 0]).all() and len({r.tobytes() for r in batch}) == 5


def test_images_at_any_byte_offset():
    """a device pointer that is not 4-byte aligned (and an image whose size is no multiple of 4): the head and tail bytes of the
    staged rows take the byte path and the result has the bits of the aligned call"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    H, W = 12, 43
    a, b, mp, mg = _kinds(H, W, "both")
    want = native(a, b, mp, mg)
    lib = _lib.lib()
    N = a.shape[0]

    def shifted(x, off):
        flat = torch.zeros(x.size + off, dtype=torch.uint8, device=G.dev())        # exactly as long as the data: nothing behind it
        flat[off:] = torch.from_numpy(x.reshape(-1)).to(G.dev())
        return flat, C.c_void_p(flat.data_ptr() + off)
    keep = [shifted(a, 1), shifted(b, 3), shifted(mp, 2), shifted(mg, 1)]
    out = torch.empty(N, 3, 3, dtype=torch.float64, device=G.dev())
    ws = torch.empty(lib.hedit_pixel_metrics_workspace_bytes(N, H, W), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_pixel_metrics(keep[0][1], keep[1][1], keep[2][1], keep[3][1], N, H, W, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                       _lib.cur_stream()))
    G.sync()
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_errors_come_before_any_launch():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib.lib()
    H, W = 64, 64
    a = torch.zeros(65, H, W, 3, dtype=torch.uint8, device=G.dev())
    out = torch.full((65, 3, 3), -7.0, dtype=torch.float64, device=G.dev())
    need = lib.hedit_pixel_metrics_workspace_bytes(64, H, W)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=G.dev())

    def call(N, h, w, ws_bytes=need, pred=a):
        return lib.hedit_pixel_metrics(_lib.ptr(pred), _lib.ptr(a), None, None, N, h, w, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.cur_stream())
    short = lib.hedit_pixel_metrics_workspace_bytes(2, H, W) - 1
    for what, bad in (("H = 10", lambda: call(1, 10, 64)), ("W = 10", lambda: call(1, 64, 10)), ("N = 0", lambda: call(0, H, W)),
                      ("N = 65", lambda: call(65, H, W)), ("short workspace", lambda: call(2, H, W, short)),
                      ("null image", lambda: call(1, H, W, pred=None))):
        rc = bad()
        msg = lib.hedit_last_error().decode()
        print(f"[pixel errors] {what}: rc {rc}, {msg!r}")
        assert rc != 0 and "bad argument" in msg and "pixel_metrics" in msg, (what, rc, msg)
        with pytest.raises(_lib.HipError, match="pixel_metrics"):
            _lib.check(rc)
    G.sync()
    assert (out == -7.0).all() and (ws == 0x5A).all()                              # nothing ran
    assert call(1, H, W) == 0
    G.sync()
    assert (out[0, 0] == torch.tensor([0.0, float("inf"), 1.0], dtype=torch.float64, device=G.dev())).all() and (out[1:] == -7.0).all()


def test_wrapper_groups_and_nan_rows():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    H, W = 12, 43
    a, b = PR.pair(H, W, "smooth")
    m = PR.rect_mask(H, W)
    m3 = m[:, :, None].repeat(3, axis=2).astype(np.float64)
    s = NativePixelMetrics(device=G.dev())
    got = s.scores([(a, b), (a, b, m3, m3), (a, b, m), (a, b, None, m), (a, a, m, m)])
    assert s.calls == 1
    for g, mode in zip(got[:4], ("none", "both", "pred", "gt")):
        _check_against_restatement(g, PR.expected(H, W, "smooth", mode), f"wrapper masks={mode}")
    assert (got[4][:, 0] == 0.0).all() and np.isposinf(got[4][:, 1]).all() and (got[4][:, 2] == 1.0).all()
    assert s.score("ssim", a, b) == got[0][0, 2] and s.score("psnr", a, b, m3, m3) == got[1][1, 1]
    assert s.score("mse", a, b, 1 - m3, 1 - m3) == got[1][2, 0]                    # the evaluator's unedit call = the unedit row
    n0 = s.calls
    many = s.scores([(a, b, m, m)] * 65)                                          # 64 + 1: two native calls
    assert s.calls == n0 + 2 and all(x.tobytes() == got[1].tobytes() for x in many)


def test_evaluator_grouped_end_to_end(tmp_path):
    """stand-in scorers, 5 synthetic 64 x 64 entries, all eighteen routed columns: --batch 4 and --batch 1 write the same bytes"""
    from PIL import Image
    from evaluation import evaluation as EV
    from hedit.clip_score import NativeClip
    from hedit.dino_score import NativeDinoStructure
    from hedit.lpips_score import NativeSqueezeLpips
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    clip = NativeClip.from_standin(width=128, layers=2, heads=2, patch_size=14, input_resolution=56, embed_dim=32, text_width=128, text_layers=2,
                                   seed=3, device=G.dev())
    lpips = NativeSqueezeLpips(device=G.dev(), seed=1)
    dino = NativeDinoStructure(device=G.dev(), seed=1, resolution=40, width=128, layers=3)
    pixel = NativePixelMetrics(device=G.dev())
    d = tmp_path / "data" / "annotation_images" / "0_x"
    out = tmp_path / "res" / "0_x"
    d.mkdir(parents=True)
    out.mkdir(parents=True)
    mapping, images = {}, {}
    for i in range(5):
        s8, t8 = (np.ascontiguousarray(x[:, :64]) for x in PR.pair(64, 64 + i, "smooth"))
        Image.fromarray(s8).save(d / f"{i}.png")
        Image.fromarray(t8).save(out / f"{i}.png")
        images[f"00{i}"] = (s8, t8)
        mapping[f"00{i}"] = dict(image_path=f"0_x/{i}.png", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a bench",
                                 editing_type_id="0", mask=[64 * 16, 64 * (8 + 4 * i)] if i != 3 else [0, 64 * 64])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    metrics = [b + p for b in ("psnr", "mse", "ssim", "lpips", "structure_distance") for p in ("", "_unedit_part", "_edit_part")] + \
        ["clip_similarity_source_image", "clip_similarity_target_image", "clip_similarity_target_image_edit_part"]
    argv = ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "h_edit",
            "--tgt_folders", str(tmp_path / "res"), "--device", "cuda", "--metrics"] + metrics
    data = {}
    for batch in (1, 4):
        res = tmp_path / f"b{batch}.csv"
        n0 = pixel.calls
        assert EV.main(argv + ["--result_path", str(res), "--batch", str(batch)], clip=clip, lpips=lpips, dino=dino, pixel=pixel) == 5
        data[batch] = (open(res, "rb").read(), pixel.calls - n0)
    assert data[1][0] == data[4][0]
    assert data[4][1] == 2 and data[1][1] == 5 * 9 - 3                             # one native call per group; per column otherwise
    rows = list(csv.reader(open(tmp_path / "b4.csv")))
    assert rows[0] == ["file_id"] + [f"h_edit|{m}" for m in metrics] and [r[0] for r in rows[1:]] == [f"00{i}" for i in range(5)]
    for r in rows[1:]:
        s8, t8 = images[r[0]]
        i = int(r[0])
        mask = EV.mask_decode(mapping[r[0]]["mask"], (64, 64)).astype(np.uint8)
        ref = PR.metrics(s8, t8, mask, mask)
        for j, base in enumerate(("psnr", "mse", "ssim")):
            for k, (part, row) in enumerate((("", 0), ("_unedit_part", 2), ("_edit_part", 1))):
                v = r[1 + 3 * j + k]
                if i == 3 and part == "_unedit_part":
                    assert v == "nan"
                    continue
                want = ref[row, ("mse", "psnr", "ssim").index(base)]
                assert abs(float(v) - want) <= {"mse": 1e-9 * want, "psnr": 1e-8, "ssim": 1e-10}[base], (r[0], base, part, v, want)
        assert all(v != "nan" for v in r[10:]) or i == 3
