"""Host side of the CLIP score (hedit/clip_score.py, csrc/clipimg.hip; no GPU): the fp32 torch restatement of the image
tower (tests/helpers/clipimg_ref.py, what the GPU tests use at sizes without a recorded vector) against
tests/golden/g20_clipimg.npz -- vectors recorded by RUNNING the reference's CLIP and transformers' CLIPModel --,
``preprocess_pil`` against CLIPImageProcessor's recorded pixel_values, the name maps, the loaders' refusals, the
evaluator's routing and the declared exports.

Restatement limits: MEASURED on the build host (fp32 torch, 8 threads) relative L2 of the restatement from the recorded
vectors, and the limit = 4 x that figure, the margin for the BLAS thread order of other hosts:
  reference CLIP encode_image, 17 tokens (fp32 vs fp32)   measured 3.65e-7   limit 1.5e-6
  transformers image features, 17 tokens (fp32 vs fp64)   measured 5.29e-7   limit 2.1e-6
  transformers image features, 257 tokens (fp32 vs fp64)  measured 4.66e-7   limit 1.9e-6
(the ViT-L/14 vector is not restated on the host: a full-size network does not belong in this suite.)
``preprocess_pil`` reproduces the recorded pixel_values bit for bit on the build host; the limit, 1e-6 absolute, is four
ulps of the largest value (|x| < 2.7, ulp 2.4e-7) for a numpy whose float64 -> float32 rounding or division differs.
"""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import clipimg_ref as CR  # noqa: E402
from helpers import text_ref as TR  # noqa: E402
from helpers.tiny import hash_normal  # noqa: E402
from hedit import clip_score as CS  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LIMITS = {"ref17": 1.5e-6, "hf17": 2.1e-6, "hf257": 1.9e-6}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g20_clipimg.npz")), json.load(open(os.path.join(GOLD, "g20_clipimg.json")))


def test_device_hash_is_the_host_hash():
    for shape, seed in (((7, 5), 3), ((1000,), 99991), ((2, 3, 4, 4), 0)):
        assert torch.equal(CR.hash_normal_t(shape, seed), hash_normal(shape, seed).float())


def test_restatement_matches_the_recorded_vectors(gold):
    g, meta = gold
    torch.manual_seed(0)
    figures = {}
    for tag, cfg, key in (("ref17", CR.TOY17, "ref_image"), ("hf17", CR.TOY17, "hf_image17"), ("hf257", CR.TOY257, "hf_image257")):
        tokens = 17 if cfg is CR.TOY17 else 257
        x = CR.test_images(meta[f"n{tokens}"], cfg["input_resolution"], meta[f"seed{tokens}"])
        with torch.no_grad():
            out = CR.image_forward(CR.clipimg_weights(**cfg), x, cfg["heads"])
        figures[tag] = TR.rel_l2(out, torch.from_numpy(g[key]))
    print("[clipimg restatement]", {k: f"{v:.2e}" for k, v in figures.items()})
    for tag, err in figures.items():
        assert err < LIMITS[tag], (tag, err)
    # the fixture is self-consistent: the two real modules agree, and the stored cosines are those of the stored features
    assert TR.rel_l2(torch.from_numpy(g["ref_image"]), torch.from_numpy(g["hf_image17"])) < 2e-6
    assert TR.rel_l2(torch.from_numpy(g["ref_text"]), torch.from_numpy(g["hf_text"])) < 2e-6
    for tokens in (17, 257):
        cos = CR.cosines(torch.from_numpy(g[f"hf_image{tokens}"]), torch.from_numpy(g["hf_text"]))
        assert float((cos - torch.from_numpy(g[f"hf_cos{tokens}"])).abs().max()) < 1e-12
    assert float((torch.from_numpy(g["ref_cos"]).double() - torch.from_numpy(g["hf_cos17"])).abs().max()) < 1e-5
    assert g["l14_image"].shape == (1, 768) and np.isfinite(g["l14_image"]).all() and g["l14_image"].std() > 0.01


def test_preprocess_pil_is_the_image_processor(gold):
    g, meta = gold
    from PIL import Image
    for i, (h, w) in enumerate(meta["proc_shapes"]):
        a = g[f"proc_in{i}"]
        assert a.shape == (h, w, 3) and np.array_equal(a, CR.uint8_image(h, w, meta["proc_seeds"][i]))
        for inp in (a, Image.fromarray(a)):
            out = CS.preprocess_pil(inp, meta["proc_size"])
            assert out.shape == (3, meta["proc_size"], meta["proc_size"]) and out.dtype == np.float32
            d = float(np.abs(out - g[f"proc_out{i}"]).max())
            assert d < 1e-6, (i, d)
    # a tall image: the crop comes from the middle of the long edge
    tall = np.zeros((90, 30, 3), dtype=np.uint8)
    tall[30:60] = 255
    out = CS.preprocess_pil(tall, 30)
    assert out.shape == (3, 30, 30) and np.allclose(out[0], (1.0 - CS.CLIP_MEAN[0]) / CS.CLIP_STD[0], atol=1e-6)
    with pytest.raises(ValueError, match="uint8"):
        CS.preprocess_pil(np.zeros((8, 8, 3), dtype=np.float32), 4)


def test_hf_name_map_round_trip_on_a_real_clipmodel():
    from transformers import CLIPConfig, CLIPModel
    v, t = CR.TOY17, TR.TOY
    c = CLIPConfig(text_config=dict(vocab_size=64, hidden_size=t["width"], intermediate_size=4 * t["width"], num_hidden_layers=1,
                                    num_attention_heads=t["heads"], max_position_embeddings=8, hidden_act="quick_gelu"),
                   vision_config=dict(hidden_size=v["width"], intermediate_size=4 * v["width"], num_hidden_layers=v["layers"],
                                      num_attention_heads=v["heads"], image_size=v["input_resolution"], patch_size=v["patch_size"],
                                      hidden_act="quick_gelu"), projection_dim=v["embed_dim"])
    sd = CLIPModel(c).state_dict()
    mapped = CS.hf_vision_to_clip_names(sd, v["layers"])
    want = CS.clipimg_param_shapes(v["width"], v["layers"], v["patch_size"], v["input_resolution"], v["embed_dim"])
    assert {k: tuple(x.shape) for k, x in mapped.items()} == want          # the text tower, logit_scale and position_ids are gone
    back = CR.clip_to_hf_vision(mapped)
    for k, x in back.items():
        assert torch.equal(x, sd[k]), k
    assert set(back) == {k for k in sd if k.startswith("vision_model.") and not k.endswith("position_ids")} | {"visual_projection.weight"}
    # q, k, v in that order
    q = sd["vision_model.encoder.layers.1.self_attn.q_proj.weight"]
    assert torch.equal(mapped["visual.transformer.resblocks.1.attn.in_proj_weight"][:v["width"]], q)
    assert torch.equal(mapped["visual.proj"], sd["visual_projection.weight"].t())
    enc = CS.NativeClipImage.from_hf_state_dict(sd, c.vision_config, device="cpu")
    assert (enc.width, enc.layers, enc.heads, enc.tokens, enc.embed_dim) == (128, 3, 2, 17, 32)
    with pytest.raises(RuntimeError, match="HIP executor only"):
        enc(torch.zeros(1, 3, 56, 56))


def test_loaders_refuse_by_name():
    w = CR.clipimg_weights(**CR.TOY17)
    enc = CS.NativeClipImage.from_clip_state_dict(dict(w, logit_scale=torch.zeros(()), positional_embedding=torch.zeros(77, 128)), device="cpu")
    assert enc.patch_size == 14 and enc.input_resolution == 56 and enc.heads == 2 and list(enc.state_dict()) == list(enc.param_shapes)
    bad = dict(w)
    del bad["visual.ln_post.bias"]
    with pytest.raises(KeyError, match="visual.ln_post.bias"):
        CS.NativeClipImage.from_clip_state_dict(bad, device="cpu")
    with pytest.raises(KeyError, match="unexpected"):
        CS.NativeClipImage.from_clip_state_dict(dict(w, **{"visual.extra": torch.zeros(1)}), device="cpu")
    with pytest.raises(ValueError, match="expected shape"):
        CS.NativeClipImage.from_clip_state_dict(dict(w, **{"visual.ln_pre.weight": torch.zeros(64)}), device="cpu")
    with pytest.raises(NotImplementedError, match="ResNets"):
        CS.NativeClipImage.from_clip_state_dict(dict(w, **{"visual.layer1.0.conv1.weight": torch.zeros(1)}), device="cpu")
    hf = CR.clip_to_hf_vision(w)
    cfg = dict(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, patch_size=14, image_size=56, hidden_act="quick_gelu")
    with pytest.raises(NotImplementedError, match="hidden_act 'gelu'"):
        CS.NativeClipImage.from_hf_state_dict(hf, dict(cfg, hidden_act="gelu"), device="cpu")
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        CS.NativeClipImage.from_hf_state_dict(hf, dict(cfg, num_attention_heads=4), device="cpu")
    part = {k: x for k, x in hf.items() if "layers.0.self_attn.k_proj.weight" not in k}
    with pytest.raises(KeyError, match="resblocks.0.attn.in_proj_weight"):
        CS.NativeClipImage.from_hf_state_dict(part, cfg, device="cpu")
    with pytest.raises(NotImplementedError, match="at most 577"):
        CS.NativeClipImage(64, 1, 1, 14, 350, 32)
    with pytest.raises(NotImplementedError, match="head dimension 64"):
        CS.NativeClipImage(96, 1, 1, 14, 56, 32)
    with pytest.raises(FileNotFoundError, match="config.json"):
        CS.NativeClip.from_pretrained(os.path.join(ROOT, "tests", "golden"))
    with pytest.raises(ValueError, match="not one embedding space"):
        CS.NativeClip(types.SimpleNamespace(embed_dim=32), types.SimpleNamespace(proj_dim=64), None)


def test_prompts_are_cut_with_the_eos_kept():
    from hedit.text import WordTokenizer
    tok = WordTokenizer()
    text = types.SimpleNamespace(proj_dim=32, context_length=77)
    clip = CS.NativeClip(types.SimpleNamespace(embed_dim=32), text, tok)
    ids = clip.tokenize(["a cat", " ".join(f"w{i}" for i in range(100)), ""])
    assert ids.shape == (3, 77) and ids.dtype == torch.int64
    assert ids[0].tolist() == [tok.bos_token_id, 1, 2] + [tok.eos_token_id] * 74
    assert ids[1, 0] == tok.bos_token_id and ids[1, -1] == tok.eos_token_id and (ids[1, 1:-1] < tok.bos_token_id).all()
    assert ids[2].tolist() == [tok.bos_token_id] + [tok.eos_token_id] * 76


class FakeClip:
    def __init__(self):
        self.seen = []

    def score(self, img, txt):
        self.seen.append((np.array(img), txt))
        return 12.5


def test_evaluator_routes_images_prompts_and_masks():
    from PIL import Image
    from evaluation import evaluation as EV
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
    mask = np.zeros((16, 16, 3))
    mask[4:9] = 1
    fake = FakeClip()
    mc = EV.MetricsCalculator("cuda", clip=fake)
    args = (Image.fromarray(src), Image.fromarray(tgt), mask, mask, "a cat", "a dog")
    assert EV.calculate_metric(mc, "clip_similarity_source_image", *args) == 12.5
    assert EV.calculate_metric(mc, "clip_similarity_target_image", *args) == 12.5
    assert EV.calculate_metric(mc, "clip_similarity_target_image_edit_part", *args) == 12.5
    (a, ta), (b, tb), (c, tc) = fake.seen
    assert np.array_equal(a, src) and ta == "a cat"
    assert np.array_equal(b, tgt) and tb == "a dog"
    assert c.dtype == np.uint8 and np.array_equal(c, np.uint8(tgt * mask)) and tc == "a dog" and (c[:4] == 0).all() and np.array_equal(c[4:9], tgt[4:9])
    assert EV.calculate_metric(mc, "clip_similarity_target_image_edit_part", args[0], args[1], mask, np.zeros_like(mask), "a", "b") == "nan"
    assert len(fake.seen) == 3
    # the other network metrics stay refused with a CLIP model present, and everything is refused without one
    for m in ("local_clip", "structure_distance", "lpips_unedit_part"):
        with pytest.raises(NotImplementedError):
            EV.calculate_metric(mc, m, *args)
    for m in ("clip_similarity_source_image", "clip_similarity_target_image", "clip_similarity_target_image_edit_part"):
        with pytest.raises(NotImplementedError, match="CLIP ViT-L/14 weights"):
            EV.calculate_metric(EV.MetricsCalculator(), m, *args)
    with pytest.raises(NotImplementedError, match="clip_path"):
        EV.MetricsCalculator().calculate_clip_similarity(args[0], "a")
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.MetricsCalculator("cpu", clip=fake)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.load_clip("/nonexistent", None, "cpu")
    ns = EV.build_parser().parse_args(["--clip_path", "d", "--clip_tokenizer", "t"])
    assert ns.clip_path == "d" and ns.clip_tokenizer == "t" and EV.build_parser().parse_args([]).clip_path is None


def test_new_exports_are_declared():
    from hedit import _lib
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    declared = set(re.findall(r"\b(hedit_clipimg_[a-z0-9_]+)\s*\(", hdr))
    want = {"hedit_clipimg_" + s for s in ("create", "destroy", "num_params", "param_name", "param_shape", "load", "missing", "finalize",
                                           "set_slices", "workspace_bytes", "encode")}
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith("hedit_clipimg_")}
    assert re.search(r"typedef struct \{ int width, layers, heads, patch_size, input_resolution, embed_dim; \} hedit_clipimg_cfg;", hdr)
    assert [f[0] for f in _lib.ClipImgCfg._fields_] == ["width", "layers", "heads", "patch_size", "input_resolution", "embed_dim"]
    assert CS.MAX_BATCH == int(re.search(r"#define HEDIT_CLIPIMG_MAX_BATCH (\d+)", hdr).group(1))
