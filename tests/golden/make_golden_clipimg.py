#!/usr/bin/env python3
"""Writes tests/golden/g20_clipimg.npz + g20_clipimg.json: expected outputs of the CLIP image tower, the text tower beside
it and the image processor, produced by RUNNING the real modules (build container only; the tests read the stored arrays):

  ref_*   the reference's clip_guidance/clip/model.py ``CLIP`` (UNMODIFIED, imported under the torchvision / ftfy stubs of
          make_golden.py's gen_clip) with toy towers, fp32 (its LayerNorm casts to float32): ``encode_image`` at 17 tokens
          (56 px, patch 14), ``encode_text``, and ``logits_per_image / logit_scale`` -- the cosines.
  hf_*    transformers' CLIPModel at the same toy size on the same weights, fp64: ``get_image_features`` at 17 tokens AND
          at 257 tokens (224 px, patch 14: the tiled softmax of csrc/clipimg.hip crosses two tile boundaries),
          ``get_text_features``, and the cosines of both image sets against the texts.
  l14_*   CLIPVisionModelWithProjection at the ViT-L/14 vision shape (width 1024, 24 layers, 16 heads, 257 tokens,
          embedding 768), one image, fp64; only the 768-float embedding is stored (rounded to fp32).
  proc_*  CLIPImageProcessor's ``pixel_values`` (shortest edge and crop 28) for two small uint8 images, one of them
          non-square, stored with the inputs.

Weights are helpers.clipimg_ref.clipimg_weights / helpers.text_ref.text_weights and images helpers.clipimg_ref.test_images
(functions of names, shapes and seeds), so nothing but ids, the uint8 inputs and the outputs is stored.

    python tests/golden/make_golden_clipimg.py            # rewrites the two files
    python tests/golden/make_golden_clipimg.py --check    # recomputes and compares with the stored arrays, bit for bit
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_STYLE = "/root/reference/text-guided-n-style"
for p in (os.path.join(ROOT, "h-edit_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from helpers import clipimg_ref as CR  # noqa: E402
from helpers.text_ref import TOY, clip_to_hf, text_weights, word_ids  # noqa: E402

SEED17, SEED257, SEEDL14 = 501, 502, 503
N17, N257 = 3, 3
PROC_SIZE = 28


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def meta_table():
    V, L = TOY["vocab_size"], TOY["context_length"]
    bos, eot = V - 2, V - 1
    ids = []
    for n, seed in ((4, 41), (L - 2, 42), (9, 43)):                       # short, all 77 positions, medium
        ids.append([bos] + word_ids(n, seed, 1, bos) + [eot] * (L - 1 - n))
    return dict(toy17=CR.TOY17, toy257=CR.TOY257, l14=CR.L14, text=TOY, ids=ids, bos=bos, eot=eot, seed17=SEED17, seed257=SEED257,
                seedl14=SEEDL14, n17=N17, n257=N257, proc_size=PROC_SIZE, proc_shapes=[[37, 53], [64, 64]], proc_seeds=[61, 62])


def gen_reference(meta):
    class _T:
        def __init__(self, *a, **k):
            pass
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Normalize=_T, ToTensor=_T, Compose=_T, Resize=_T, CenterCrop=_T,
                          InterpolationMode=types.SimpleNamespace(BICUBIC=3))
    _stub("ftfy", fix_text=lambda s: s)
    sys.path.insert(0, REF_STYLE)
    from clip_guidance.clip import model as cm
    t, v = meta["text"], meta["toy17"]
    clip = cm.CLIP(embed_dim=v["embed_dim"], image_resolution=v["input_resolution"], vision_layers=v["layers"], vision_width=v["width"],
                   vision_patch_size=v["patch_size"], context_length=t["context_length"], vocab_size=t["vocab_size"],
                   transformer_width=t["width"], transformer_heads=t["heads"], transformer_layers=t["layers"])
    assert clip.visual.transformer.resblocks[0].attn.num_heads == v["heads"]
    w = dict(text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"]))
    w.update(CR.clipimg_weights(**v))
    own = dict(clip.named_parameters())
    assert set(own) - {"logit_scale"} == set(w), sorted(set(own) ^ set(w))[:8]
    with torch.no_grad():
        for name, val in w.items():
            assert tuple(own[name].shape) == tuple(val.shape), name
            own[name].copy_(val)
    clip.eval()
    ids = torch.tensor(meta["ids"], dtype=torch.int64)
    img = CR.test_images(meta["n17"], v["input_resolution"], meta["seed17"])
    with torch.no_grad():
        fi, ft = clip.encode_image(img), clip.encode_text(ids)
        logits, _ = clip(img, ids)
        cos = logits / clip.logit_scale.exp()
    return {"ref_image": fi.numpy().astype(np.float32), "ref_text": ft.numpy().astype(np.float32), "ref_cos": cos.numpy().astype(np.float32)}


def _feat(x):
    return x if torch.is_tensor(x) else x.pooler_output


def hf_clip(v, t):
    from transformers import CLIPConfig, CLIPModel
    c = CLIPConfig(text_config=dict(vocab_size=t["vocab_size"], hidden_size=t["width"], intermediate_size=4 * t["width"],
                                    num_hidden_layers=t["layers"], num_attention_heads=t["heads"],
                                    max_position_embeddings=t["context_length"], hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                    attention_dropout=0.0, bos_token_id=t["vocab_size"] - 2, eos_token_id=2, pad_token_id=1,
                                    projection_dim=v["embed_dim"]),
                   vision_config=dict(hidden_size=v["width"], intermediate_size=4 * v["width"], num_hidden_layers=v["layers"],
                                      num_attention_heads=v["heads"], image_size=v["input_resolution"], patch_size=v["patch_size"],
                                      hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0, projection_dim=v["embed_dim"]),
                   projection_dim=v["embed_dim"])
    m = CLIPModel(c).eval()
    own = m.state_dict()
    wt = text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"])
    proj = wt.pop("text_projection")
    sd = clip_to_hf(wt, "text_model.")
    sd["text_projection.weight"] = proj.t().contiguous()
    sd.update(CR.clip_to_hf_vision(CR.clipimg_weights(**v)))
    for k in own:
        if k.endswith("position_ids") or k == "logit_scale":
            sd[k] = own[k]
    m.load_state_dict(sd, strict=True)
    return m.to(torch.float64)


def gen_hf(meta):
    out = {}
    ids = torch.tensor(meta["ids"], dtype=torch.int64)
    for tag, v, n, seed in (("17", meta["toy17"], meta["n17"], meta["seed17"]), ("257", meta["toy257"], meta["n257"], meta["seed257"])):
        m = hf_clip(v, meta["text"])
        img = CR.test_images(n, v["input_resolution"], seed).double()
        with torch.no_grad():
            fi = _feat(m.get_image_features(pixel_values=img))
            ft = _feat(m.get_text_features(input_ids=ids))
        out[f"hf_image{tag}"] = fi.numpy().astype(np.float64)
        out[f"hf_cos{tag}"] = CR.cosines(fi, ft).numpy().astype(np.float64)
        if "hf_text" in out:
            assert np.array_equal(out["hf_text"], ft.numpy())             # the text tower does not see the image size: stored once
        out["hf_text"] = ft.numpy().astype(np.float64)
    return out


def gen_l14(meta):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    v = meta["l14"]
    c = CLIPVisionConfig(hidden_size=v["width"], intermediate_size=4 * v["width"], num_hidden_layers=v["layers"],
                         num_attention_heads=v["heads"], image_size=v["input_resolution"], patch_size=v["patch_size"], hidden_act="quick_gelu",
                         layer_norm_eps=1e-5, attention_dropout=0.0, projection_dim=v["embed_dim"])
    m = CLIPVisionModelWithProjection(c).eval()
    own = m.state_dict()
    sd = CR.clip_to_hf_vision(CR.clipimg_weights(**v))
    for k in own:
        if k.endswith("position_ids"):
            sd[k] = own[k]
    m.load_state_dict(sd, strict=True)
    del sd
    m = m.to(torch.float64)
    img = CR.test_images(1, v["input_resolution"], meta["seedl14"]).double()
    with torch.no_grad():
        e = m(pixel_values=img).image_embeds
    return {"l14_image": e.numpy().astype(np.float32)}


def gen_proc(meta):
    from PIL import Image
    from transformers import CLIPImageProcessor
    s = meta["proc_size"]
    proc = CLIPImageProcessor(size={"shortest_edge": s}, crop_size={"height": s, "width": s})
    out = {}
    for i, ((h, w), seed) in enumerate(zip(meta["proc_shapes"], meta["proc_seeds"])):
        a = CR.uint8_image(h, w, seed)
        pv = proc(images=Image.fromarray(a), return_tensors="np")["pixel_values"][0]
        assert pv.shape == (3, s, s), pv.shape
        out[f"proc_in{i}"] = a
        out[f"proc_out{i}"] = np.asarray(pv, dtype=np.float32)
    return out


def main():
    torch.set_num_threads(8)
    if not os.path.isdir(REF_STYLE):
        raise SystemExit("reference tree not present")
    meta = meta_table()
    d = gen_proc(meta)                  # before the reference: transformers must not see the torchvision stub
    d.update(gen_hf(meta))
    d.update(gen_l14(meta))
    d.update(gen_reference(meta))
    npz, js = os.path.join(HERE, "g20_clipimg.npz"), os.path.join(HERE, "g20_clipimg.json")
    if "--check" in sys.argv:
        old = np.load(npz)
        bad = [k for k in d if k not in old.files or old[k].dtype != d[k].dtype or not np.array_equal(old[k], d[k])]
        bad += [k for k in old.files if k not in d]
        if json.load(open(js)) != json.loads(json.dumps(meta)):
            bad.append("g20_clipimg.json")
        print("g20_clipimg: identical" if not bad else f"g20_clipimg: DIFFERENT {bad}")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(npz, **d)
    with open(js, "w") as f:
        json.dump(meta, f)
    print({k: (v.shape, str(v.dtype)) for k, v in d.items()}, os.path.getsize(npz))


if __name__ == "__main__":
    main()
