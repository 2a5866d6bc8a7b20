"""CPU tests of the local_clip plumbing: the template loader, the prompt de-duplication of NativeLocalClip.scores (with a fake
NativeClip that records its calls; the head launch itself is a GPU matter and is replaced), and the evaluator's routing,
refusals and flags with a fake scorer."""
import csv
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hedit import local_clip_score as LC  # noqa: E402

TEMPLATES = ["a photo of a {}.", "a sketch of the {}.", "{} in the rain."]


def test_template_loader(tmp_path):
    good = tmp_path / "t.txt"
    good.write_text("# my templates\n\na photo of a {}.\n   a sketch of the {}.  \n{} in the rain.\n\n", encoding="utf-8")
    assert LC.load_templates(str(good)) == TEMPLATES == LC.NativeLocalClip.load_templates(str(good))
    uni = tmp_path / "u.txt"
    uni.write_text("une photo d’un {} été\n", encoding="utf-8")
    assert LC.load_templates(str(uni)) == ["une photo d’un {} été"]
    for body, line in (("a photo.\n", 1), ("ok {}\n{} and {}\n", 2), ("# c\nok {}\n\na {0} b\n", 4), ("a {} }\n", 1)):
        bad = tmp_path / "bad.txt"
        bad.write_text(body, encoding="utf-8")
        with pytest.raises(ValueError, match=rf"bad\.txt:{line}\b"):
            LC.load_templates(str(bad))
    empty = tmp_path / "e.txt"
    empty.write_text("# nothing\n\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no templates"):
        LC.load_templates(str(empty))
    with pytest.raises(ValueError, match="templates"):
        LC.NativeLocalClip(None, [])
    with pytest.raises(ValueError, match="exactly one"):
        LC.NativeLocalClip(None, ["no brace"])
    with pytest.raises(ValueError, match="256"):
        LC.NativeLocalClip(None, ["{}"] * 257)


class FakeNativeClip:
    """text_features: a vector that is a function of the prompt alone; every call is recorded"""

    def __init__(self):
        self.text_calls = []
        self.image = types.SimpleNamespace(device=torch.device("cpu"), input_resolution=16)

    def text_features(self, prompts):
        self.text_calls.append(list(prompts))
        return torch.tensor([[float(len(p)), float(sum(map(ord, p)) % 97), 1.0, 0.0] for p in prompts])


def test_each_distinct_prompt_is_encoded_once(monkeypatch):
    clip = FakeNativeClip()
    lc = LC.NativeLocalClip(clip, TEMPLATES)
    seen, real_direction = {}, LC.direction
    monkeypatch.setattr(lc, "_images", lambda images: torch.arange(len(images) * 4, dtype=torch.float32).reshape(len(images), 4))

    def fake_direction(txt, img):
        seen["txt"], seen["img"] = txt, img
        return torch.arange(txt.shape[0], dtype=torch.float64)

    monkeypatch.setattr(LC, "direction", fake_direction)
    items = [("i0", "a cat", "j0", "a dog"), ("i1", "a cat", "j1", "a dog"), ("i2", "a bird", "j2", "a cat")]
    assert lc.scores(items) == [0.0, 1.0, 2.0] and lc.calls == 1
    # three distinct prompts x three templates, prompt-major, in order of first appearance: ONE text call
    want = [t.format(p) for p in ("a cat", "a dog", "a bird") for t in TEMPLATES]
    assert clip.text_calls == [want]
    assert seen["txt"].shape == (3, 2, 3, 4) and seen["img"].shape == (3, 2, 4)
    f = clip.text_features
    assert torch.equal(seen["txt"][0, 0], f([t.format("a cat") for t in TEMPLATES])) and torch.equal(seen["txt"][0], seen["txt"][1])
    assert torch.equal(seen["txt"][2, 0], f([t.format("a bird") for t in TEMPLATES])) and torch.equal(seen["txt"][2, 1], seen["txt"][0, 0])
    assert torch.equal(seen["img"].flatten(), torch.arange(24, dtype=torch.float32))          # source then target, item by item
    # more template prompts than one text call takes: chunks of at most 256, the same rows
    clip.text_calls.clear()
    many = LC.NativeLocalClip(clip, ["{} %d" % i for i in range(100)])
    monkeypatch.setattr(many, "_images", lambda images: torch.zeros(len(images), 4))
    many.scores(items)
    assert [len(c) for c in clip.text_calls] == [256, 44] and clip.text_calls[0][:2] == ["a cat 0", "a cat 1"]
    assert torch.equal(seen["txt"][2, 0], f(["a bird %d" % i for i in range(100)]))
    # `score` is `scores` of one item; without a GPU the image side refuses
    lc2 = LC.NativeLocalClip(clip, TEMPLATES)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lc2.score(np.zeros((8, 8, 3), np.uint8), "a", np.zeros((8, 8, 3), np.uint8), "b")
    with pytest.raises(RuntimeError, match="no CPU path"):
        real_direction(torch.zeros(1, 2, 1, 4), torch.zeros(1, 2, 4))


class FakeLocalClip:
    def __init__(self):
        self.seen, self.score_calls, self.scores_calls = [], 0, 0

    def _value(self, a, sp, b, tp):
        self.seen.append((np.array(a), sp, np.array(b), tp))
        return float(int(np.array(a)[0, 0, 0]) - int(np.array(b)[0, 0, 0])) / 256.0 + len(sp) - len(tp)

    def score(self, a, sp, b, tp):
        self.score_calls += 1
        return self._value(a, sp, b, tp)

    def scores(self, items):
        self.scores_calls += 1
        return [self._value(*it) for it in items]


def test_evaluator_routes_the_four_arguments_and_ignores_masks():
    from evaluation import evaluation as EV
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
    mask = np.zeros((16, 16, 3))
    mask[4:9] = 1
    fake = FakeLocalClip()
    mc = EV.MetricsCalculator("cuda", local_clip=fake)
    args = (Image.fromarray(src), Image.fromarray(tgt), mask, mask, "a cat", "a big dog")
    v = EV.calculate_metric(mc, "local_clip", *args)
    a, sp, b, tp = fake.seen[0]
    assert np.array_equal(a, src) and np.array_equal(b, tgt) and (sp, tp) == ("a cat", "a big dog") and fake.score_calls == 1
    assert v == fake._value(src, "a cat", tgt, "a big dog")
    # masks are ignored: an empty mask (the nan rule of the masked columns) changes nothing, and neither does the keyword
    assert EV.calculate_metric(mc, "local_clip", args[0], args[1], np.zeros_like(mask), np.zeros_like(mask), "a cat", "a big dog") == v
    assert mc.compute_local_clip(args[0], "a cat", args[1], "a big dog", mask=mask) == v
    # refused without the scorer, with or without the other models, and on the CPU
    for other in (EV.MetricsCalculator(), EV.MetricsCalculator("cuda", clip=object())):
        with pytest.raises(NotImplementedError, match=r"--clip_path.*--local_clip_templates"):
            EV.calculate_metric(other, "local_clip", *args)
        with pytest.raises(NotImplementedError, match=r"--clip_path.*--local_clip_templates"):
            other.compute_local_clip(args[0], "a", args[1], "b")
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.MetricsCalculator("cpu", local_clip=fake)
    # the other network metrics stay refused with only this scorer present
    for m in ("lpips", "structure_distance", "clip_similarity_source_image"):
        with pytest.raises(NotImplementedError):
            EV.calculate_metric(mc, m, *args)


def _dataset(tmp_path, n=3, S=16):
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
        mapping[f"k{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a " + "b" * i,
                                editing_type_id="0", mask=[S * 4, S * 5])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    return ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "m0", "m1",
            "--tgt_folders", str(tmp_path / "res0"), str(tmp_path / "res1")]


def test_a_group_is_one_scores_call(tmp_path):
    from evaluation import evaluation as EV
    argv = _dataset(tmp_path) + ["--device", "cuda", "--metrics", "local_clip"]
    runs = {}
    for batch in (1, 4):
        fake = FakeLocalClip()
        res = tmp_path / f"b{batch}.csv"
        assert EV.main(argv + ["--result_path", str(res), "--batch", str(batch)], local_clip=fake) == 3
        runs[batch] = (open(res, "rb").read(), fake)
    assert runs[1][0] == runs[4][0]
    assert runs[1][1].score_calls == 6 and runs[1][1].scores_calls == 0
    assert runs[4][1].scores_calls == 2 and runs[4][1].score_calls == 0 and len(runs[4][1].seen) == 6      # 6 pairs in groups of 4
    rows = list(csv.reader(open(tmp_path / "b4.csv")))
    assert rows[0] == ["file_id", "m0|local_clip", "m1|local_clip"] and len(rows) == 4
    assert runs[4][1].seen[0][1] == "a cat on a bench" and runs[4][1].seen[2][3] == "a dog on a b"
    # a scorer without `scores` is called item by item
    inner = FakeLocalClip()
    one = types.SimpleNamespace(score=inner.score)
    res = tmp_path / "s.csv"
    EV.main(argv + ["--result_path", str(res), "--batch", "4"], local_clip=one)
    assert inner.score_calls == 6 and open(res, "rb").read() == runs[1][0]


def test_flags(tmp_path):
    from evaluation import evaluation as EV
    ns = EV.build_parser().parse_args([])
    assert ns.local_clip_templates is None and ns.native_preprocess is False
    argv = _dataset(tmp_path, n=1)
    tpl = tmp_path / "t.txt"
    tpl.write_text("a photo of a {}.\n", encoding="utf-8")
    with pytest.raises(SystemExit) as e:
        EV.main(argv + ["--device", "cuda", "--local_clip_templates", str(tpl), "--result_path", str(tmp_path / "x.csv")])
    assert "--clip_path" in str(e.value) and "--local_clip_templates" in str(e.value)
    with pytest.raises(SystemExit) as e:
        EV.main(argv + ["--device", "cuda", "--native_preprocess", "--result_path", str(tmp_path / "x.csv")])
    assert "--clip_path" in str(e.value) and "--native_preprocess" in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.main(argv + ["--device", "cpu", "--native_preprocess", "--clip_path", "/nonexistent", "--result_path", str(tmp_path / "x.csv")])
    # --local_clip_templates with a CLIP object: the scorer is built from the file, and --native_preprocess switches the object
    clip = types.SimpleNamespace(native_preprocess=False, score=lambda img, txt: 1.0)
    built = {}

    class Probe(FakeLocalClip):
        def __init__(self, c, templates):
            super().__init__()
            built["clip"], built["templates"] = c, templates

    import hedit.local_clip_score as mod
    orig = mod.NativeLocalClip
    mod.NativeLocalClip = Probe
    try:
        res = tmp_path / "y.csv"
        assert EV.main(argv + ["--device", "cuda", "--local_clip_templates", str(tpl), "--native_preprocess", "--metrics", "local_clip",
                               "--result_path", str(res)], clip=clip) == 1
    finally:
        mod.NativeLocalClip = orig
    assert built["clip"] is clip and built["templates"] == ["a photo of a {}."] and clip.native_preprocess is True
    assert len(list(csv.reader(open(res)))[1]) == 3


def test_the_end_to_end_reference_meets_its_own_condition():
    """the fp64 restatement tests/test_gpu_local_clip.py compares with: its derived limit is at most 0.05 on the chosen seeds
    and prompts, and the head's restatement gives 0 for equal images and NaN for equal prompts"""
    from helpers import local_clip_ref as R
    ref = R.reference()
    assert np.isfinite(ref["value"]) and abs(ref["value"]) <= 1 and 0 < ref["limit"] <= R.LIMIT_CEILING, ref
    assert ref["limit"] == 8 * R.DELTA * (1 / ref["norm_e"] + 1 / ref["norm_d"])
    g = torch.Generator().manual_seed(2)
    txt, img = torch.randn(2, 2, 3, 8, generator=g), torch.randn(2, 2, 8, generator=g)
    img[0, 1] = img[0, 0]
    txt[1, 1] = txt[1, 0]
    got = R.direction_ref(txt, img)
    assert got[0] == 0.0 and torch.isnan(got[1])
