"""CPU tests of the native pixel-metrics path: the fp64 restatement (tests/helpers/pixel_ref.py) against the evaluator's torch
code, the host-side refusals of hedit.pixel_score, the evaluator's --native_pixel / --batch wiring with fake scorers, and
the ABI bookkeeping.

The restatement-vs-torch limits are 4 x the gap first measured on a CPU (pixel_ref.GAP_*: mse 1.4e-7 relative, psnr 5.9e-6 dB,
ssim 1.4e-5 absolute), the margin covering another host's convolution kernels.  RE-MEASURED on this repository's CPU host over
the same shapes and inputs: mse 1.5e-7, psnr 3.2e-6 dB, ssim 1.2e-5.
"""
import csv
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import pixel_ref as PR  # noqa: E402
from hedit import pixel_score as PS  # noqa: E402


def _gaps(got, ref):
    """(mse relative, psnr dB, ssim absolute) between two (mse, psnr, ssim) triples"""
    e0 = abs(got[0] - ref[0]) / ref[0] if ref[0] else abs(got[0])
    e1 = 0.0 if got[1] == ref[1] else abs(got[1] - ref[1])
    return e0, e1, abs(got[2] - ref[2])


def test_taps_are_the_evaluators_window():
    """GAUSS_TAPS (and PM_TAPS of the kernel, the same literals) are fp32 values whose outer product is _gauss(): bit for bit on
    a host whose fp32 exp agrees, and never further than one fp32 ulp per tap (1.2e-7 relative, so 2.4e-7 on a product)"""
    from evaluation import evaluation as EV
    taps = np.array(PS.GAUSS_TAPS)
    assert len(taps) == 11 and np.array_equal(taps, taps.astype(np.float32).astype(np.float64)) and np.array_equal(taps, taps[::-1])
    want = EV._gauss().double().numpy()
    got = np.outer(taps, taps)
    assert np.abs(got - want).max() <= 2.5e-7 * want.max() and np.abs(got / want - 1).max() <= 2.5e-7
    src = open(os.path.join(ROOT, "h-edit_amd", "csrc", "pixmetrics.hip")).read()
    lits = re.search(r"#define PM_TAPS \{(.*?)\}", src, re.S).group(1).replace("\\", " ")
    assert tuple(float.fromhex(v.strip()) for v in lits.split(",")) == PS.GAUSS_TAPS


@pytest.mark.parametrize("shape", PR.SHAPES + (PR.BIG,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_agrees_with_the_torch_path(shape):
    from evaluation import evaluation as EV
    H, W = shape
    mc = EV.MetricsCalculator("cpu")
    m3 = PR.rect_mask(H, W)[:, :, None].repeat(3, axis=2).astype(np.float64)      # as main builds it
    worst = [0.0, 0.0, 0.0]
    for kind in PR.KINDS:
        a, b = PR.pair(H, W, kind)
        ref = PR.expected(H, W, kind)
        for p, (ma, mb) in enumerate(((None, None), (m3, m3), (1 - m3, 1 - m3))):
            got = (mc.calculate_mse(a, b, ma, mb), mc.calculate_psnr(a, b, ma, mb), mc.calculate_ssim(a, b, ma, mb))
            worst = [max(w, e) for w, e in zip(worst, _gaps(got, ref[p]))]
        one = PR.expected(H, W, kind, "pred")[1]                                  # only one of the two masks: the edit part
        got = (mc.calculate_mse(a, b, m3, None), mc.calculate_psnr(a, b, m3, None), mc.calculate_ssim(a, b, m3, None))
        worst = [max(w, e) for w, e in zip(worst, _gaps(got, one))]
    print(f"[pixel ref vs torch] {H} x {W}: mse {worst[0]:.2e} relative, psnr {worst[1]:.2e} dB, ssim {worst[2]:.2e}")
    assert worst[0] <= PR.GAP_MSE_REL and worst[1] <= PR.GAP_PSNR_DB and worst[2] <= PR.GAP_SSIM, worst


def test_restatement_on_equal_images_and_without_masks():
    a, _ = PR.pair(12, 43, "noise")
    r = PR.metrics(a, a, PR.rect_mask(12, 43), PR.rect_mask(12, 43))
    assert (r[:, 0] == 0.0).all() and np.isposinf(r[:, 1]).all() and (r[:, 2] == 1.0).all()
    r = PR.expected(12, 43, "noise", "none")
    assert np.isfinite(r[0]).all() and np.isnan(r[1:]).all()


def test_refusals():
    m = PS.NativePixelMetrics()                      # nothing touches the GPU before the host checks
    a, b = PR.pair(12, 43, "noise")
    mask = PR.rect_mask(12, 43)
    with pytest.raises(ValueError, match="binary masks only.*torch path"):
        m.scores([(a, b, mask * 2, mask)])
    with pytest.raises(ValueError, match="binary masks only.*torch path"):
        m.score("mse", a, b, None, mask.astype(np.float64) * 0.5)
    m3 = mask[:, :, None].repeat(3, axis=2)
    m3[3, 9, 1] ^= 1
    with pytest.raises(ValueError, match="not channel-identical"):
        m.scores([(a, b, m3, m3)])
    with pytest.raises(ValueError, match="at least 11 x 11"):
        m.scores([(a[:10], b[:10])])
    with pytest.raises(ValueError, match="at least 11 x 11"):
        m.score("ssim", a[:, :10], b[:, :10])
    with pytest.raises(ValueError, match="one image size"):
        m.scores([(a, b), (a[:11], b[:11])])
    with pytest.raises(ValueError, match="unknown metric"):
        m.score("lpips", a, b)
    with pytest.raises(ValueError, match="uint8"):
        m.scores([(a.astype(np.float32), b)])
    assert m.scores([]) == [] and m.calls == 0
    cpu = PS.NativePixelMetrics(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        cpu.scores([(a, b)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        cpu.score("mse", a, b)
    t = torch.zeros(1, 12, 43, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.metrics(t, t)
    assert np.array_equal(PS.mask_u8(mask[:, :, None].repeat(3, axis=2).astype(np.float64), 12, 43), mask)


class FakePixel:
    """a pixel scorer with both entry points: a made-up, deterministic function of the masked images"""

    def __init__(self):
        self.score_calls, self.scores_calls, self.items = 0, 0, []

    @staticmethod
    def _row(a, b, m):
        a, b = np.array(a).astype(np.float64) * m[:, :, None], np.array(b).astype(np.float64) * m[:, :, None]
        return [float(((a - b) ** 2).mean()), float(np.abs(a - b).mean()), float((a * b).mean())]

    def scores(self, items):
        self.scores_calls += 1
        out = []
        for it in items:
            it = tuple(it) + (None,) * (4 - len(it))
            self.items.append(it)
            H, W = np.array(it[0]).shape[:2]
            r = np.full((3, 3), np.nan)
            r[0] = self._row(it[0], it[1], np.ones((H, W)))
            if it[2] is not None:
                m = PS.mask_u8(it[2], H, W).astype(np.float64)
                r[1], r[2] = self._row(it[0], it[1], m), self._row(it[0], it[1], 1 - m)
            out.append(r)
        return out

    def score(self, metric, img_pred, img_gt, mask_pred=None, mask_gt=None):
        self.score_calls += 1
        H, W = np.array(img_pred).shape[:2]
        m = np.ones((H, W)) if mask_pred is None else PS.mask_u8(mask_pred, H, W).astype(np.float64)
        return self._row(img_pred, img_gt, m)[PS.METRICS.index(metric)]


class FakePairScorer:
    """lpips / dino stand-in; `batched` decides whether it has ``scores``"""

    def __init__(self, scale):
        self.scale, self.score_calls, self.scores_calls = scale, 0, 0

    def _one(self, a, b, ma=None, mb=None):
        a, b = np.array(a).astype(np.float64), np.array(b).astype(np.float64)
        a, b = (a if ma is None else a * ma), (b if mb is None else b * mb)
        return self.scale * float(np.abs(a - b).mean())

    def score(self, a, b, ma=None, mb=None):
        self.score_calls += 1
        return self._one(a, b, ma, mb)


class FakeBatchedPairScorer(FakePairScorer):
    def scores(self, items):
        self.scores_calls += 1
        return [self._one(*it) for it in items]


class FakeClip:
    def __init__(self):
        self.score_calls, self.scores_calls = 0, 0

    def score(self, image, text):
        self.score_calls += 1
        return float(np.array(image).astype(np.float64).mean()) + len(text)

    def scores(self, images, texts):
        self.scores_calls += 1
        return [float(np.array(i).astype(np.float64).mean()) + len(t) for i, t in zip(images, texts)]


ALL_COLUMNS = [b + p for b in ("psnr", "mse", "ssim", "lpips", "structure_distance") for p in ("", "_unedit_part", "_edit_part")] + \
    ["clip_similarity_source_image", "clip_similarity_target_image", "clip_similarity_target_image_edit_part"]


def _dataset(tmp_path, n=5, S=24):
    """n entries x 2 methods of S x S images; entry 1 has no mask run at all (the decoded mask is the one-pixel border: every
    rule passes), entry 2 a mask covering everything (unedit columns nan), and mask_decode cannot give an empty mask (its
    border is forced to 1), so the edit nan rule is driven through evaluate_group directly below"""
    from PIL import Image
    src = tmp_path / "data" / "annotation_images" / "0_x"
    src.mkdir(parents=True)
    outs = [tmp_path / f"res{k}" / "0_x" for k in range(2)]
    for o in outs:
        o.mkdir(parents=True)
    rng = np.random.default_rng(11)
    mapping = {}
    for i in range(n):
        name = f"{i}.png"
        Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8)).save(src / name)
        for o in outs:
            Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8)).save(o / name)
        mask = [S * 6, S * 9] if i not in (1, 2) else ([] if i == 1 else [0, S * S])
        mapping[f"k{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a " + "b" * i,
                                editing_type_id="0", mask=mask)
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    return ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "m0", "m1",
            "--tgt_folders", str(tmp_path / "res0"), str(tmp_path / "res1"), "--device", "cuda"]


def test_grouped_run_writes_the_same_bytes(tmp_path):
    from evaluation import evaluation as EV
    argv = _dataset(tmp_path) + ["--metrics"] + ALL_COLUMNS
    runs = {}
    for batch in (1, 3):
        sc = dict(clip=FakeClip(), lpips=FakeBatchedPairScorer(0.5), dino=FakePairScorer(2.0), pixel=FakePixel())
        res = tmp_path / f"b{batch}.csv"
        assert EV.main(argv + ["--result_path", str(res), "--batch", str(batch)], **sc) == 5
        runs[batch] = (open(res, "rb").read(), sc)
    assert runs[1][0] == runs[3][0]
    rows = list(csv.reader(open(tmp_path / "b3.csv")))
    assert [r[0] for r in rows[1:]] == [f"k{i}" for i in range(5)] and all(len(r) == 1 + 2 * 18 for r in rows)
    head = rows[0][1:19]
    full = rows[3]                                                               # entry 2: the mask covers everything
    assert [full[1 + head.index(f"m0|{b}_unedit_part")] for b in ("psnr", "mse", "ssim", "lpips", "structure_distance")] == ["nan"] * 5
    assert all(v != "nan" for r in (rows[1], rows[2]) for v in r[1:])
    one, three = runs[1][1], runs[3][1]
    # --batch 1 is the per-image loop: no batched entry point is touched
    assert one["pixel"].scores_calls == 0 and one["pixel"].score_calls == 10 * 9 - 2 * 3
    assert one["clip"].scores_calls == 0 and one["lpips"].scores_calls == 0
    # --batch 3 over 10 pairs: 4 groups; the pixel scorer ONCE per group, the others once per column and group
    assert three["pixel"].scores_calls == 4 and three["pixel"].score_calls == 0 and len(three["pixel"].items) == 10
    assert three["clip"].scores_calls == 4 * 3 and three["clip"].score_calls == 0
    assert three["lpips"].scores_calls == 4 * 3 and three["lpips"].score_calls == 0
    assert three["dino"].score_calls == one["dino"].score_calls == 10 * 3 - 2          # no `scores`: item by item
    # a scorer object with `score` only (the fakes of the older tests) still works for the pixel columns
    class ScoreOnly:
        def __init__(self):
            self.inner = FakePixel()

        def score(self, *a):
            return self.inner.score(*a)
    res = tmp_path / "score_only.csv"
    EV.main(argv[:-18] + ["psnr", "mse_unedit_part", "ssim_edit_part", "--result_path", str(res), "--batch", "4"], pixel=ScoreOnly())
    want = [[r[0]] + [r[1 + k * 18 + head.index(f"m0|{c}")] for k in range(2) for c in ("psnr", "mse_unedit_part", "ssim_edit_part")] for r in rows[1:]]
    assert list(csv.reader(open(res)))[1:] == want


def test_group_applies_every_nan_rule_before_the_scorers():
    from PIL import Image
    from evaluation import evaluation as EV
    rng = np.random.default_rng(3)
    img = [Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)) for _ in range(2)]
    some = np.zeros((16, 16, 3))
    some[4:9] = 1
    masks = [some, np.zeros_like(some), np.ones_like(some)]
    items = [dict(src=img[0], tgt=img[1], mask=m, src_p="a cat", tgt_p="a dog") for m in masks]
    sc = dict(clip=FakeClip(), lpips=FakeBatchedPairScorer(0.5), dino=FakePairScorer(2.0), pixel=FakePixel())
    mc = EV.MetricsCalculator("cuda", **sc)
    got = EV.evaluate_group(mc, ALL_COLUMNS, items)
    ref = dict(clip=FakeClip(), lpips=FakeBatchedPairScorer(0.5), dino=FakePairScorer(2.0), pixel=FakePixel())
    mr = EV.MetricsCalculator("cuda", **ref)
    want = [[EV.calculate_metric(mr, c, it["src"], it["tgt"], it["mask"], it["mask"], it["src_p"], it["tgt_p"]) for c in ALL_COLUMNS] for it in items]
    assert got == want
    edit = [i for i, c in enumerate(ALL_COLUMNS) if c.endswith("_edit_part")]
    unedit = [i for i, c in enumerate(ALL_COLUMNS) if c.endswith("_unedit_part")]
    assert all(got[1][i] == "nan" for i in edit) and all(got[2][i] == "nan" for i in unedit)
    assert not any(v == "nan" for v in got[0]) and sc["pixel"].scores_calls == 1
    # the empty mask reaches the pixel scorer for its live unedit part only as a binary mask, never as a nan'd request
    assert sc["lpips"].scores_calls == 3 and sc["clip"].scores_calls == 3


def test_evaluator_flags_and_defaults(tmp_path):
    from PIL import Image
    from evaluation import evaluation as EV
    ns = EV.build_parser().parse_args([])
    assert ns.batch == 1 and ns.native_pixel is False
    argv = _dataset(tmp_path, n=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.main(argv[:-2] + ["--device", "cpu", "--native_pixel", "--result_path", str(tmp_path / "x.csv")])
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.load_pixel("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.MetricsCalculator("cpu", pixel=FakePixel())
    with pytest.raises(SystemExit):
        EV.main(argv + ["--batch", "0", "--result_path", str(tmp_path / "x.csv")])
    # without `pixel` the calculator is today's torch code: the values of the formulas, unchanged by the new keyword
    a, b = PR.pair(12, 43, "smooth")
    m3 = PR.rect_mask(12, 43)[:, :, None].repeat(3, axis=2).astype(np.float64)
    mc = EV.MetricsCalculator()
    assert mc.pixel is None
    x, y = EV._pair(Image.fromarray(a), Image.fromarray(b), m3, m3)
    assert mc.calculate_mse(Image.fromarray(a), Image.fromarray(b), m3, m3) == float(((x - y) ** 2).mean())
    x, y = EV._pair(a, b, None, None)
    assert mc.calculate_psnr(a, b) == float(10.0 * torch.log10(1.0 / ((x - y) ** 2).mean()))
    assert abs(mc.calculate_ssim(a, b, m3, m3) - PR.expected(12, 43, "smooth")[1, 2]) <= PR.GAP_SSIM
    fake = FakePixel()
    mp = EV.MetricsCalculator("cuda", pixel=fake)
    assert mp.calculate_mse(a, b, m3, m3) == fake._row(a, b, PR.rect_mask(12, 43).astype(np.float64))[0] and fake.score_calls == 1
    # a default --batch 1 run on the CPU still writes the torch values
    res = tmp_path / "cpu.csv"
    assert EV.main(argv[:-2] + ["--result_path", str(res)]) == 1
    assert len(list(csv.reader(open(res)))[1]) == 1 + 2 * 3


def test_new_exports_are_declared():
    from hedit import _lib
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    want = {"hedit_pixel_metrics", "hedit_pixel_metrics_workspace_bytes"}
    assert set(re.findall(r"\b(hedit_pixel_[a-z0-9_]+)\s*\(", hdr)) == want == {n for n in _lib.EXPORTS if n.startswith("hedit_pixel_")}
    assert PS.MAX_BATCH == int(re.search(r"#define HEDIT_PIXEL_METRICS_MAX_BATCH (\d+)", hdr).group(1)) == 64
    assert os.path.exists(_lib.LIB_PATH), "build libhedit_hip.so first: python h-edit_amd/build.py"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in want)
    ws = _lib.lib().hedit_pixel_metrics_workspace_bytes
    assert ws(1, 11, 11) == 6 * 8 and ws(5, 75, 53) == 5 * 6 * 2 * 5 * 8 and ws(1, 512, 512) == 6 * 16 * 32 * 8
    assert ws(0, 64, 64) == 0 and ws(65, 64, 64) == 0 and ws(1, 10, 64) == 0 and ws(1, 64, 10) == 0
