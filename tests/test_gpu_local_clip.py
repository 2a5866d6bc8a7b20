"""-m gpu: the local_clip metric on the native executors -- the direction head (hedit_clip_direction of csrc/imgprep.hip) against
a torch float64 restatement, the whole metric (hedit.local_clip_score.NativeLocalClip on a tiny stand-in CLIP) against the
float64 restatement of tests/helpers/local_clip_ref.py, and the evaluator's column.

Limits.  Head: 1e-12 absolute -- fp64 sums of about 800 O(1) terms err by at most roughly 1e-13, the limit is ten times that.
Whole metric: 8 delta (1 / |b^ - a^| + 1 / |d|) with delta = 1e-4, the towers' parity limit, computed from the reference's own
quantities (local_clip_ref.reference; at most 0.05 by tests/test_host_local_clip.py).  Batch and storage comparisons are bit
for bit.  Every test prints its figures with -s before it asserts.

MEASURED (MI355X, bfloat16 build): head 0 / 5.6e-17 / 2.1e-17 from float64 torch at (1, 1, 8) / (5, 3, 64) / (2, 80, 768); whole
metric 0.258028 against the reference's 0.258030 (|e| 0.2397, |d| 0.8617): 1.2e-6 of a limit of 4.27e-3.  Wall time of the file
under 1 s.
"""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers import imgprep_ref as IR  # noqa: E402
from helpers import local_clip_ref as R  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.clip_score import NativeClip, NativeClipImage  # noqa: E402
from hedit.local_clip_score import NativeLocalClip, direction  # noqa: E402
from hedit.text import NativeClipText  # noqa: E402

HEAD_LIMIT = 1e-12


@pytest.fixture(scope="module")
def scorer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wi, wt = R.weights()
    tok = R.tokenizer()
    clip = NativeClip(NativeClipImage.from_clip_state_dict(wi, device=G.dev()),
                      NativeClipText.from_clip_state_dict(wt, device=G.dev(), eos_token_id=tok.eos_token_id), tok)
    return NativeLocalClip(clip, R.TEMPLATES)


def _features(P, T, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, 2, T, E, generator=g), torch.randn(P, 2, E, generator=g)


@pytest.mark.parametrize("shape", [(1, 1, 8), (5, 3, 64), (2, 80, 768)], ids=lambda s: "P%d-T%d-E%d" % s)
def test_head_against_float64(shape):
    P, T, E = shape
    txt, img = _features(P, T, E, 100 + E)
    got = direction(txt.to(G.dev()), img.to(G.dev())).cpu()
    want = R.direction_ref(txt, img)
    err = float((got - want).abs().max())
    print(f"[direction head] P {P}, T {T}, E {E}: values {want.min():.4f} .. {want.max():.4f}, max abs from float64 torch {err:.3e}")
    assert got.dtype == torch.float64 and torch.isfinite(got).all() and err <= HEAD_LIMIT


def test_head_special_values_and_batch_invariance():
    txt, img = _features(5, 3, 64, 7)
    img[1, 1] = img[1, 0]                                                # equal image features: exactly 0.0
    txt[3, 1] = txt[3, 0]                                                # equal prompt features: the reference's 0 / 0
    t, i = txt.to(G.dev()), img.to(G.dev())
    got = direction(t, i).cpu()
    assert got[1] == 0.0 and not np.signbit(float(got[1])) and torch.isnan(got[3])
    live = [0, 2, 4]
    assert torch.isfinite(got[live]).all() and float((got[live] - R.direction_ref(txt, img)[live]).abs().max()) <= HEAD_LIMIT
    singles = torch.cat([direction(t[p:p + 1], i[p:p + 1]) for p in range(5)]).cpu()
    assert np.array_equal(got.numpy(), singles.numpy(), equal_nan=True)                             # bit for bit


def test_head_errors_are_reported_before_the_launch():
    lib = _lib.lib()
    txt, img = _features(2, 3, 8, 9)
    t, i = txt.to(G.dev()), img.to(G.dev())
    out = torch.full((2,), -7.0, dtype=torch.float64, device=G.dev())

    def call(t=t, i=i, P=2, T=3, E=8, o=out):
        return lib.hedit_clip_direction(_lib.ptr(t), _lib.ptr(i), P, T, E, _lib.ptr(o), _lib.cur_stream())

    for kw, msg in ((dict(t=None), "null"), (dict(i=None), "null"), (dict(o=None), "null"), (dict(P=0), "1 <= P <= 64"), (dict(P=65), "1 <= P <= 64"),
                    (dict(T=0), "1 <= T <= 256"), (dict(T=257), "1 <= T <= 256"), (dict(E=6), "multiple of 4"), (dict(E=0), "multiple of 4"),
                    (dict(E=4100), "at most 4096")):
        rc = call(**kw)
        err = lib.hedit_last_error().decode()
        assert rc == -1 and "clip_direction" in err and msg in err, (kw, rc, err)
    G.sync()
    assert (out == -7.0).all()                                           # nothing ran
    assert call() == 0
    G.sync()
    assert float((out.cpu() - R.direction_ref(txt, img)).abs().max()) <= HEAD_LIMIT
    with pytest.raises(ValueError, match="expected float32"):
        direction(t.double(), i)


def test_the_whole_metric_against_float64(scorer):
    ref = R.reference()
    a, b = R.images()
    got = scorer.score(a, R.PROMPTS[0], b, R.PROMPTS[1])
    print(f"[local_clip] reference {ref['value']:.6f} (|e| {ref['norm_e']:.4f}, |d| {ref['norm_d']:.4f}), native {got:.6f}: "
          f"abs {abs(got - ref['value']):.3e}, limit {ref['limit']:.3e}")
    assert ref["limit"] <= R.LIMIT_CEILING
    assert abs(got - ref["value"]) <= ref["limit"]
    from PIL import Image
    assert scorer.score(Image.fromarray(a), R.PROMPTS[0], Image.fromarray(b), R.PROMPTS[1]) == got
    assert scorer.score(a, R.PROMPTS[0], a, R.PROMPTS[1]) == 0.0         # the same image twice
    assert np.isnan(scorer.score(a, R.PROMPTS[0], b, R.PROMPTS[0]))      # the same prompt twice


def test_scores_is_the_score_loop(scorer):
    imgs = [IR.image(56, 40, 60 + k) for k in range(6)]
    items = [(imgs[0], R.PROMPTS[0], imgs[1], R.PROMPTS[1]), (imgs[2], "a red car", imgs[3], "a blue car parked outside"),
             (imgs[4], R.PROMPTS[0], imgs[5], R.PROMPTS[1])]
    clip = scorer.clip
    n_txt, n_img, n_head = clip.text.calls, clip.image.calls, scorer.calls
    batched = scorer.scores(items)
    # four distinct prompts x three templates in ONE text call, six images in ONE image call, ONE head launch
    assert (clip.text.calls, clip.image.calls, scorer.calls) == (n_txt + 1, n_img + 1, n_head + 1)
    loop = [scorer.score(*it) for it in items]
    print(f"[local_clip] 3 items: {batched}")
    assert batched == loop and all(np.isfinite(v) and abs(v) <= 1 for v in batched) and len(set(batched)) == 3


def test_evaluator_column_and_native_preprocess(scorer, tmp_path):
    from PIL import Image
    from evaluation import evaluation as EV
    src = tmp_path / "data" / "annotation_images" / "0_x"
    src.mkdir(parents=True)
    outs = [tmp_path / f"res{k}" / "0_x" for k in range(2)]
    mapping = {}
    for o in outs:
        o.mkdir(parents=True)
    for i in range(3):
        name = f"{i}.png"
        Image.fromarray(IR.image(40, 40, 70 + i)).save(src / name)
        for k, o in enumerate(outs):
            Image.fromarray(IR.image(40, 40, 80 + 10 * k + i)).save(o / name)
        mapping[f"k{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a bench " + "now " * i,
                                editing_type_id="0", mask=[40 * 10, 40 * 12])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    metrics = ["local_clip", "clip_similarity_target_image", "clip_similarity_target_image_edit_part"]
    argv = ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "m0", "m1",
            "--tgt_folders", str(tmp_path / "res0"), str(tmp_path / "res1"), "--device", "cuda", "--metrics"] + metrics
    clip = scorer.clip
    runs = {}
    try:
        for tag, extra in (("b1", ["--batch", "1"]), ("b4", ["--batch", "4"]), ("native", ["--batch", "1", "--native_preprocess"]),
                           ("native4", ["--batch", "4", "--native_preprocess"])):
            res = tmp_path / f"{tag}.csv"
            clip.native_preprocess = False
            assert EV.main(argv + ["--result_path", str(res)] + extra, clip=clip, local_clip=scorer) == 3
            assert clip.native_preprocess is ("native" in tag)
            runs[tag] = open(res, "rb").read()
    finally:
        clip.native_preprocess = False
    assert runs["b1"] == runs["b4"] == runs["native"] == runs["native4"]
    rows = list(csv.reader(open(tmp_path / "b1.csv")))
    assert rows[0] == ["file_id"] + [f"{k}|{m}" for k in ("m0", "m1") for m in metrics] and [r[0] for r in rows[1:]] == ["k0", "k1", "k2"]
    for r in rows[1:]:
        vals = [float(v) for v in r[1:]]
        print(f"[evaluator] {r[0]}: {vals}")
        assert all(np.isfinite(v) for v in vals) and abs(vals[0]) <= 1 and abs(vals[3]) <= 1 and vals[0] != vals[3]
    # without the scorer the column stays refused, by name
    with pytest.raises(NotImplementedError, match="local_clip_templates"):
        EV.main(argv + ["--result_path", str(tmp_path / "x.csv")], clip=clip)
    # a template file on the command line builds the same scorer on the same towers
    tpl = tmp_path / "templates.txt"
    tpl.write_text("# made up for this test\n" + "\n".join(R.TEMPLATES) + "\n", encoding="utf-8")
    res = tmp_path / "file.csv"
    assert EV.main(argv + ["--result_path", str(res), "--local_clip_templates", str(tpl)], clip=clip) == 3
    assert open(res, "rb").read() == runs["b1"]
