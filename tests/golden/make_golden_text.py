#!/usr/bin/env python3
"""Writes tests/golden/g19_text.npz + g19_text.json: expected outputs of the CLIP text transformer, produced by RUNNING
the real modules (build container only; the tests read the stored arrays):

  ref_*   the reference's clip_guidance/clip/model.py ``CLIP`` (UNMODIFIED, imported under the torchvision / ftfy stubs of
          make_golden.py's gen_clip) with a toy text tower: ``encode_text`` (pooled at argmax, times text_projection) and the
          ln_final hidden states, fp32 (its LayerNorm casts to float32, so it cannot run in fp64 unmodified).  Ids as
          its ``clip.tokenize`` lays them out: BOS, words, EOT (the highest id), zeros.
  hf_hidden, hfa_pooled   transformers' CLIPTextModel at the same size on the same weights (minus text_projection),
          hidden_act "quick_gelu", config eos_token_id = 2: the legacy rule, pooled at argmax.  fp64.
  hfe_pooled   the same module with the real EOS id configured: pooled at the first EOS (same hidden states, checked
          here).  Ids padded with the EOS id, as SD's tokenizer pads; the EOS id is NOT the highest id here, so the two
          rules pick different rows.  fp64.
  sd_*    CLIPTextModel at SD-1.x width (768, 12 heads, 12 layers, context 77) with a 1024-row vocabulary, two prompts,
          computed in fp64 and stored rounded to fp32.

Weights are helpers.text_ref.text_weights (a function of parameter name and shape), so nothing but ids and outputs is stored.

    python tests/golden/make_golden_text.py            # rewrites the two files
    python tests/golden/make_golden_text.py --check    # recomputes and compares with the stored arrays, bit for bit
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

from helpers.text_ref import SDW, TOY, clip_to_hf, text_weights, word_ids  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def ids_table():
    V, L = TOY["vocab_size"], TOY["context_length"]
    bos, eot = V - 2, V - 1
    ref = []
    for n, seed in ((5, 11), (L - 2, 12), (0, 13)):                      # short, all 77 positions, empty
        w = word_ids(n, seed, 1, bos)
        ref.append([bos] + w + [eot] + [0] * (L - 2 - n))
    hbos, heos = 299, 300                                                 # EOS below the highest word id
    hf = []
    for n, seed in ((6, 21), (L - 2, 22), (0, 23)):
        w = word_ids(n, seed, 3, V, exclude=(hbos, heos))
        hf.append([hbos] + w + [heos] * (L - 1 - n))
    Vs = SDW["vocab_size"]
    sbos, seos = Vs - 2, Vs - 1
    sd = []
    for n, seed in ((7, 31), (23, 32)):
        w = word_ids(n, seed, 1, sbos)
        sd.append([sbos] + w + [seos] * (L - 1 - n))
    return dict(toy=TOY, sd=SDW, ref_ids=ref, ref_bos=bos, ref_eot=eot, hf_ids=hf, hf_bos=hbos, hf_eos=heos,
                sd_ids=sd, sd_bos=sbos, sd_eos=seos)


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
    t = meta["toy"]
    clip = cm.CLIP(embed_dim=t["proj_dim"], image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=32,
                   context_length=t["context_length"], vocab_size=t["vocab_size"], transformer_width=t["width"],
                   transformer_heads=t["heads"], transformer_layers=t["layers"])
    w = text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"])
    own = dict(clip.named_parameters())
    with torch.no_grad():
        for name, v in w.items():
            assert tuple(own[name].shape) == tuple(v.shape), name
            own[name].copy_(v)
    clip.eval()
    ids = torch.tensor(meta["ref_ids"], dtype=torch.int64)
    with torch.no_grad():
        pooled = clip.encode_text(ids)
        x = clip.token_embedding(ids) + clip.positional_embedding
        hidden = clip.ln_final(clip.transformer(x.permute(1, 0, 2)).permute(1, 0, 2))
    return {"ref_hidden": hidden.numpy().astype(np.float32), "ref_pooled": pooled.numpy().astype(np.float32)}


def hf_model(cfg, eos_token_id, bos_token_id, dtype):
    from transformers import CLIPTextConfig, CLIPTextModel
    c = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["width"], intermediate_size=4 * cfg["width"],
                       num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       max_position_embeddings=cfg["context_length"], hidden_act="quick_gelu", layer_norm_eps=1e-5,
                       attention_dropout=0.0, bos_token_id=bos_token_id, eos_token_id=eos_token_id, pad_token_id=eos_token_id)
    m = CLIPTextModel(c).eval()
    own = m.state_dict()
    prefix = "text_model." if any(k.startswith("text_model.") for k in own) else ""
    w = text_weights(cfg["width"], cfg["layers"], cfg["vocab_size"], cfg["context_length"], 0)
    sd = clip_to_hf(w, prefix)
    for k in own:
        if k.endswith("position_ids"):
            sd[k] = own[k]
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def gen_hf(meta):
    out = {}
    ids = torch.tensor(meta["hf_ids"], dtype=torch.int64)
    for tag, eos in (("hfa", 2), ("hfe", meta["hf_eos"])):
        m = hf_model(meta["toy"], eos, meta["hf_bos"], torch.float64)
        with torch.no_grad():
            r = m(input_ids=ids)
        out[f"{tag}_hidden"] = r.last_hidden_state.numpy().astype(np.float64)
        out[f"{tag}_pooled"] = r.pooler_output.numpy().astype(np.float64)
    assert np.array_equal(out["hfa_hidden"], out["hfe_hidden"])      # the rule only moves the pooled row: stored once
    out["hf_hidden"] = out.pop("hfa_hidden")
    del out["hfe_hidden"]
    assert not np.array_equal(out["hfa_pooled"], out["hfe_pooled"]), "the two pooling rules must pick different rows"
    ids = torch.tensor(meta["sd_ids"], dtype=torch.int64)
    m = hf_model(meta["sd"], 2, meta["sd_bos"], torch.float64)
    with torch.no_grad():
        r = m(input_ids=ids)
    out["sd_hidden"] = r.last_hidden_state.numpy().astype(np.float32)
    out["sd_pooled"] = r.pooler_output.numpy().astype(np.float32)
    return out


def main():
    torch.set_num_threads(4)
    torch.set_grad_enabled(True)
    if not os.path.isdir(REF_STYLE):
        raise SystemExit("reference tree not present")
    meta = ids_table()
    d = gen_hf(meta)                    # before the reference: transformers must not see the torchvision stub
    d.update(gen_reference(meta))
    npz, js = os.path.join(HERE, "g19_text.npz"), os.path.join(HERE, "g19_text.json")
    if "--check" in sys.argv:
        old = np.load(npz)
        bad = [k for k in d if k not in old.files or old[k].dtype != d[k].dtype or not np.array_equal(old[k], d[k])]
        bad += [k for k in old.files if k not in d]
        if json.load(open(js)) != json.loads(json.dumps(meta)):
            bad.append("g19_text.json")
        print("g19_text: identical" if not bad else f"g19_text: DIFFERENT {bad}")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(npz, **d)
    with open(js, "w") as f:
        json.dump(meta, f)
    print({k: (v.shape, str(v.dtype)) for k, v in d.items()}, os.path.getsize(npz))


if __name__ == "__main__":
    main()
