"""-m gpu: the native CLIP image tower (hedit_clipimg_* of csrc/clipimg.hip on the shared encoder kernels and block forward of
csrc/encoder.hip / encoder.h, behind hedit.clip_score.NativeClipImage), the
CLIP score on top of it and the evaluator's clip_similarity_* columns, against tests/golden/g20_clipimg.npz -- vectors
recorded by RUNNING the reference's ``CLIP`` and transformers' CLIPModel (tests/golden/make_golden_clipimg.py; pinned on
the host by tests/test_host_clip_score.py).

Limits.  Embeddings: 1e-4 relative L2, the limit tests/test_gpu_text.py sets for this arithmetic family (fp32 stream,
three-term split-bf16 operands, fp32 accumulation).  Scores: 0.02 absolute -- two unit vectors each within 1e-4 move a
cosine by at most 2e-4, times 100.  Batch, slice-count and storage-format comparisons are bit for bit.

MEASURED (MI355X, bfloat16 build; relative L2, every test prints its figures with -s before it asserts):
  reference CLIP, 3 layers, 17 tokens: encode_image 7.5e-6, encode_text 1.1e-5, logits_per_image / logit_scale within 3.2e-6
  transformers, 3 layers (fp64): 7.5e-6 at 17 tokens, 7.2e-6 at 257 tokens (three key tiles)
  ViT-L/14 shape, 24 layers (fp64): 9.8e-6 -- depth does not add to it; a tenth of the limit
  577 tokens, 2 layers, against torch in fp64 on the same GPU: 6.4e-6
  scores of 9 (image, prompt) pairs: within 2.7e-4 of the fixture's
The fp32 restatement on the host is 3.7e-7 ... 5.3e-7 from the same vectors (tests/test_host_clip_score.py).
Wall time of the file: 7.7 s (5.7 s inside pytest), of which the child process in the other storage build 2.3 s and the
ViT-L/14 case 0.4 s.
"""
import csv
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import clipimg_ref as CR  # noqa: E402
from helpers import gpu as G  # noqa: E402
from helpers import text_ref as TR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.clip_score import NativeClip, NativeClipImage, clipimg_param_shapes  # noqa: E402
from hedit.text import NativeClipText  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
LIMIT = 1e-4
SCORE_LIMIT = 0.02


class IdsTokenizer:
    """prompt "p<i>" -> row i of the fixture's ids up to its first EOT (the call surface NativeClip uses)"""

    def __init__(self, ids, eot):
        self.ids, self.eos_token_id = ids, eot

    def encode(self, p):
        row = self.ids[int(p[1:])]
        return row[:row.index(self.eos_token_id) + 1]


@pytest.fixture(scope="module")
def gold():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(os.path.join(GOLD, "g20_clipimg.npz")), json.load(open(os.path.join(GOLD, "g20_clipimg.json")))


@pytest.fixture(scope="module")
def towers(gold):
    """the toy image towers at 17 and 257 tokens and the toy text tower: the fixture's weights, regenerated from their names"""
    t = TR.TOY
    text = NativeClipText.from_clip_state_dict(TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"]),
                                               device=G.dev(), eos_token_id=gold[1]["eot"])
    return {17: NativeClipImage.from_clip_state_dict(CR.clipimg_weights(**CR.TOY17), device=G.dev()),
            257: NativeClipImage.from_clip_state_dict(CR.clipimg_weights(**CR.TOY257), device=G.dev()), "text": text}


def _images(meta, tokens):
    cfg = CR.TOY17 if tokens == 17 else CR.TOY257
    return CR.test_images(meta[f"n{tokens}"], cfg["input_resolution"], meta[f"seed{tokens}"])


def _report(name, got, want):
    err = G.rel_err(got, torch.from_numpy(np.asarray(want)))
    print(f"[clipimg parity] {name}: rel L2 {err:.3e}")
    return err


def test_parity_with_the_reference_clip(gold, towers):
    g, meta = gold
    enc = towers[17]
    out = enc(_images(meta, 17))
    txt = towers["text"](torch.tensor(meta["ids"]))[1]
    G.sync()
    assert out.shape == (3, 32) and out.dtype == torch.float32 and out.is_cuda
    errs = [_report("reference encode_image (17 tokens)", out, g["ref_image"]), _report("reference encode_text", txt, g["ref_text"])]
    assert max(errs) < LIMIT, errs
    cos = CR.cosines(out.cpu(), txt.cpu())
    d = float((cos - torch.from_numpy(g["ref_cos"]).double()).abs().max())
    print(f"[clipimg parity] reference logits_per_image / logit_scale: max abs {d:.3e}")
    assert 100 * d < SCORE_LIMIT
    # the C table is the Python table: names, order, shapes
    lib, h = _lib.lib(), enc._h
    want = clipimg_param_shapes(**{k: v for k, v in CR.TOY17.items() if k != "heads"})
    assert lib.hedit_clipimg_num_params(h) == len(want) and lib.hedit_clipimg_missing(h) == 0
    nd, dims = C.c_int(), (C.c_int * 4)()
    for i, (name, shape) in enumerate(want.items()):
        assert lib.hedit_clipimg_param_name(h, i).decode() == name
        _lib.check(lib.hedit_clipimg_param_shape(h, i, C.byref(nd), dims))
        assert tuple(dims[:nd.value]) == shape, name


@pytest.mark.parametrize("tokens", [17, 257])
def test_parity_with_transformers(gold, tokens):
    g, meta = gold
    cfg = CR.TOY17 if tokens == 17 else CR.TOY257
    vcfg = dict(hidden_size=cfg["width"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], patch_size=cfg["patch_size"],
                image_size=cfg["input_resolution"], hidden_act="quick_gelu", projection_dim=cfg["embed_dim"])
    enc = NativeClipImage.from_hf_state_dict(CR.clip_to_hf_vision(CR.clipimg_weights(**cfg)), vcfg, device=G.dev())
    assert enc.tokens == tokens
    out = enc(_images(meta, tokens).to(G.dev()))
    G.sync()
    assert _report(f"transformers get_image_features ({tokens} tokens, vs fp64)", out, g[f"hf_image{tokens}"]) < LIMIT


def test_parity_at_the_vit_l14_shape(gold):
    """width 1024, 24 layers, 16 heads, 257 tokens, embedding 768: the weights are generated on the device (1.2 GB), the
    expected embedding was computed once in fp64 by transformers"""
    g, meta = gold
    enc = NativeClipImage.from_clip_state_dict(CR.clipimg_weights(device=G.dev(), **CR.L14), device=G.dev())
    out = enc(CR.test_images(1, 224, meta["seedl14"], device=G.dev()))
    G.sync()
    assert out.shape == (1, 768)
    assert _report("ViT-L/14 shape, 24 layers (vs fp64)", out, g["l14_image"]) < LIMIT


def test_577_tokens_against_torch_in_fp64():
    """ViT-L/14@336's token count, the most the kernel takes: five key tiles (4 x 128 + 65) and nineteen 32-row passes, the
    last with one row.  No recorded vector at this size: the reference is the restatement the host tests pin, run in fp64
    by torch on the same GPU."""
    cfg = dict(CR.TOY17, layers=2, input_resolution=336)
    w = CR.clipimg_weights(device=G.dev(), **cfg)
    enc = NativeClipImage.from_clip_state_dict(w, device=G.dev())
    assert enc.tokens == 577
    x = CR.test_images(2, 336, 504, device=G.dev())
    out = enc(x)
    one = enc(x[1:])
    with torch.no_grad():
        want = CR.image_forward(w, x, cfg["heads"], torch.float64)
    G.sync()
    assert torch.equal(out[1:], one)
    assert _report("577 tokens, 2 layers (vs fp64 torch)", out, want.cpu().numpy()) < LIMIT
    # nineteen passes: one workgroup walks them all, or 2 / 3 / 7 / 18 share them unevenly; the default is 19
    for z in (1, 2, 3, 7, 18):
        got = enc.set_slices(z)(x)
        G.sync()
        assert torch.equal(got, out), z


def test_batch_invariance_bit_for_bit(gold, towers):
    enc = towers[257]
    x = _images(gold[1], 257)
    a, b = enc(x), enc(x)
    singles = [enc(x[i:i + 1]) for i in range(3)]
    G.sync()
    assert torch.equal(a, b) and torch.equal(a, torch.cat(singles))
    assert torch.isfinite(a).all() and a.std() > 0.01


def test_a_row_does_not_depend_on_the_slice_count(gold, towers):
    """the attention grid's z: 1 workgroup walks all nine 32-row passes of an (image, head), or 2 / 4 / 5 / 8 share them
    (9, one pass each, is the default; a count above it is clamped to it)"""
    enc = towers[257]
    x = _images(gold[1], 257)
    base = enc(x)
    try:
        for z in (1, 2, 4, 5, 8, 64):
            got = enc.set_slices(z)(x)
            G.sync()
            assert torch.equal(got, base), z
    finally:
        enc.set_slices(0)


def test_the_other_storage_build_gives_the_same_bits(gold, towers, tmp_path):
    """ONE child process in the other storage format (bf16 parent -> libhedit_hip_f16.so, and the reverse)"""
    other = "bf16" if _lib.STORAGE == "f16" else "f16"
    out = tmp_path / "child.npz"
    env = dict(os.environ, HEDIT_STORAGE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "clipimg_child.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    c = np.load(out)
    assert int(c["is_f16"][0]) == (1 if other == "f16" else 0)
    meta = gold[1]
    for tokens in (17, 257):
        mine = towers[tokens](_images(meta, tokens))
        G.sync()
        assert np.array_equal(mine.cpu().numpy(), c[f"e{tokens}"]), tokens


def test_score_against_the_fixture_and_batched_scores(gold, towers):
    g, meta = gold
    clip = NativeClip(towers[257], towers["text"], IdsTokenizer(meta["ids"], meta["eot"]))
    x = _images(meta, 257)
    want = np.maximum(100.0 * g["hf_cos257"], 0.0)
    pairs = [(i, j) for i in range(3) for j in range(3)]
    n_img, n_txt = clip.image.calls, clip.text.calls
    batched = clip.scores([x[i] for i, _ in pairs], [f"p{j}" for _, j in pairs])
    assert clip.image.calls == n_img + 1 and clip.text.calls == n_txt + 1          # one native call per tower for the whole list
    loop = [clip.score(x[i], f"p{j}") for i, j in pairs]
    d = max(abs(s - want[i, j]) for s, (i, j) in zip(batched, pairs))
    print(f"[clip score] 9 pairs, scores {min(batched):.3f} .. {max(batched):.3f}: max abs from the fixture {d:.3e}")
    assert d < SCORE_LIMIT
    assert batched == loop                                                         # bit for bit, by batch invariance
    assert any(s > 0 for s in batched) and all(s >= 0 for s in batched)
    ids = clip.tokenize(["p1"])                                                    # the prompt that fills all 77 positions
    assert ids.shape == (1, 77) and ids[0, -1] == meta["eot"]


def test_evaluator_end_to_end_with_standin_weights(tmp_path):
    from PIL import Image
    from evaluation import evaluation as EV
    clip = NativeClip.from_standin(width=128, layers=2, heads=2, patch_size=14, input_resolution=56, embed_dim=32, text_width=128, text_layers=2,
                                   seed=3, device=G.dev())
    d = tmp_path / "data" / "annotation_images" / "0_x"
    out = tmp_path / "res" / "0_x"
    d.mkdir(parents=True)
    out.mkdir(parents=True)
    mapping = {}
    for i, name in enumerate(("a.png", "b.png")):
        Image.fromarray(CR.uint8_image(64, 64, 70 + i)).save(d / name)
        Image.fromarray(CR.uint8_image(64, 64, 80 + i)).save(out / name)
        mapping[f"00{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a bench",
                                 editing_type_id="0", mask=[64 * 16, 64 * 24])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    res = tmp_path / "results.csv"
    metrics = ["clip_similarity_source_image", "clip_similarity_target_image", "clip_similarity_target_image_edit_part"]
    argv = ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "h_edit",
            "--tgt_folders", str(tmp_path / "res"), "--result_path", str(res), "--metrics"] + metrics
    assert EV.main(argv + ["--device", "cuda"], clip=clip) == 2
    rows = list(csv.reader(open(res)))
    assert rows[0] == ["file_id"] + [f"h_edit|{m}" for m in metrics] and [r[0] for r in rows[1:]] == ["000", "001"]
    for r in rows[1:]:
        vals = [float(v) for v in r[1:]]
        print(f"[evaluator] {r[0]}: {vals}")
        assert all(math.isfinite(v) and v >= 0 for v in vals)
        assert vals[2] != vals[1]                                                   # the masked image is another image
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.main(argv + ["--device", "cpu"], clip=clip)
    with pytest.raises(NotImplementedError, match="CLIP ViT-L/14 weights"):
        EV.main(argv + ["--device", "cuda"])


def test_errors_are_reported_before_anything_is_launched(gold, towers):
    enc = towers[17]
    x = _images(gold[1], 17).to(G.dev())
    ok = enc(x).clone()
    n0 = enc.calls
    with pytest.raises(ValueError, match=r"expected a float \(B, 3, 56, 56\)"):
        enc(torch.zeros(1, 3, 224, 224))
    assert enc.calls == n0
    lib, h = _lib.lib(), enc._h
    B = 3
    out = torch.full((B, 32), -7.0, device=G.dev())
    need = lib.hedit_clipimg_workspace_bytes(h, B)
    assert need > 0 and lib.hedit_clipimg_workspace_bytes(h, 0) == 0 and lib.hedit_clipimg_workspace_bytes(h, 257) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=G.dev())

    def call(B=B, img=x, o=out, w=ws, nbytes=need):
        return lib.hedit_clipimg_encode(h, _lib.ptr(img), B, _lib.ptr(o), _lib.ptr(w), nbytes, _lib.cur_stream())

    for kw, msg in ((dict(B=0), "1 <= B <= 256"), (dict(B=257), "1 <= B <= 256"), (dict(nbytes=need // 2), "workspace too small"),
                    (dict(w=None), "null workspace"), (dict(img=None), "null"), (dict(o=None), "null")):
        rc = call(**kw)                                                 # the message is that of the LAST failed call: read it right away
        assert rc == -1 and msg in lib.hedit_last_error().decode(), (kw, rc, msg, lib.hedit_last_error())
    G.sync()
    assert (out == -7.0).all()                                          # nothing ran
    assert call() == 0
    G.sync()
    assert torch.equal(out, ok)
    hh = C.c_void_p()
    for cfg, msg in ((_lib.ClipImgCfg(96, 1, 1, 14, 56, 32), "head dimension"), (_lib.ClipImgCfg(128, 1, 1, 14, 56, 32), "head dimension"),
                     (_lib.ClipImgCfg(64, 1, 1, 14, 350, 32), "577"), (_lib.ClipImgCfg(64, 1, 1, 14, 60, 32), "multiple of patch_size"),
                     (_lib.ClipImgCfg(64, 0, 1, 14, 56, 32), "positive"), (_lib.ClipImgCfg(64, 1, 1, 14, 56, 30), "multiple of 4")):
        assert lib.hedit_clipimg_create(C.byref(cfg), C.byref(hh)) == -1 and msg in lib.hedit_last_error().decode(), msg
    # 577 tokens (ViT-L/14@336) are accepted
    cfg = _lib.ClipImgCfg(64, 1, 1, 14, 336, 32)
    assert lib.hedit_clipimg_create(C.byref(cfg), C.byref(hh)) == 0
    lib.hedit_clipimg_destroy(hh)
    with pytest.raises(NotImplementedError, match="at most 577"):
        NativeClipImage(64, 1, 1, 14, 350, 32)
