"""Host side of the native prompt encoder (hedit.text.NativeClipText, csrc/text.hip).

(1) tests/helpers/text_ref.text_forward, a plain fp32 restatement of the CLIP text transformer, reproduces every vector of
tests/golden/g19_text.npz -- recorded by RUNNING the reference's ``CLIP.encode_text`` and transformers' CLIPTextModel
(tests/golden/make_golden_text.py) -- to 1e-5 relative L2: ten times the fp32-vs-fp64 distance of the real module at SD size
(7.3e-7); a wrong mask, activation, q/k/v order or pool position is an O(1) error.  That pins what the GPU tests compare
the kernels with, and the weight generator both sides share.
(2) The three loaders map transformers names (both prefixes), OpenAI names and the torch stand-in onto one native table;
mistakes in a checkpoint are reported, unsupported models are refused, bad ids are rejected before anything is launched."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import text_ref as TR  # noqa: E402
from hedit.text import ClipTextEncoder, NativeClipText, hf_to_clip_names, text_param_shapes  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G19 = os.path.join(GOLD, "g19_text.npz")
LIMIT = 1e-5


def g19():
    return np.load(G19), json.load(open(os.path.join(GOLD, "g19_text.json")))


def toy_weights(proj):
    t = TR.TOY
    return TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"] if proj else 0)


def sd_weights():
    t = TR.SDW
    return TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], 0)


def _check(name, got, want):
    err = TR.rel_l2(got, torch.from_numpy(np.asarray(want)))
    print(f"{name}: rel L2 {err:.3e}")
    assert err < LIMIT, (name, err)


def test_restatement_reproduces_the_reference_clip_vectors():
    g, meta = g19()
    assert meta["toy"] == TR.TOY and meta["sd"] == TR.SDW
    ids = torch.tensor(meta["ref_ids"])
    assert ids.shape == (3, 77) and ids[1].min() > 0 and (ids[2, 2:] == 0).all()      # short / full / empty
    assert (ids.argmax(-1) == torch.tensor([6, 76, 1])).all() and int(ids.max()) == meta["ref_eot"]
    h, p = TR.text_forward(toy_weights(True), ids, TR.TOY["heads"])
    _check("ref_hidden", h, g["ref_hidden"])
    _check("ref_pooled", p, g["ref_pooled"])


def test_restatement_reproduces_the_transformers_vectors_under_both_pooling_rules():
    g, meta = g19()
    ids = torch.tensor(meta["hf_ids"])
    eos = meta["hf_eos"]
    first = (ids == eos).int().argmax(-1)
    assert (first == torch.tensor([7, 76, 1])).all()
    assert (ids.argmax(-1) != first).any(), "the fixture must tell the two rules apart"
    w = toy_weights(False)
    h, pa = TR.text_forward(w, ids, TR.TOY["heads"])
    _, pe = TR.text_forward(w, ids, TR.TOY["heads"], eos_token_id=eos)
    _check("hf_hidden", h, g["hf_hidden"])
    _check("hfa_pooled", pa, g["hfa_pooled"])
    _check("hfe_pooled", pe, g["hfe_pooled"])
    assert TR.rel_l2(pa, torch.from_numpy(g["hfe_pooled"])) > 1e-2         # the wrong rule is an O(1) error


def test_restatement_reproduces_the_sd_width_fp64_vectors():
    g, meta = g19()
    ids = torch.tensor(meta["sd_ids"])
    h, p = TR.text_forward(sd_weights(), ids, TR.SDW["heads"])
    _check("sd_hidden", h, g["sd_hidden"])
    _check("sd_pooled", p, g["sd_pooled"])


def test_exchanged_q_and_k_are_far_outside_the_limit():
    g, meta = g19()
    ids = torch.tensor(meta["hf_ids"])
    w = toy_weights(False)
    sw = dict(w)
    k = "transformer.resblocks.0.attn.in_proj_weight"
    q, kk, v = w[k].chunk(3, dim=0)
    sw[k] = torch.cat([kk, q, v])
    h, _ = TR.text_forward(sw, ids, TR.TOY["heads"])
    assert TR.rel_l2(h, torch.from_numpy(g["hf_hidden"])) > 1e-2


# ---------------------------------------------------------------------------------------------- loaders
def _same_table(enc, want):
    assert list(enc.params) == list(want) == list(enc.param_shapes)
    for k in want:
        assert torch.equal(enc.params[k], want[k]), k


def test_hf_names_with_and_without_prefix_map_onto_the_native_table():
    t = TR.TOY
    w = toy_weights(False)
    cfg = dict(hidden_size=t["width"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"], vocab_size=t["vocab_size"],
               max_position_embeddings=t["context_length"], hidden_act="quick_gelu", eos_token_id=2)
    for prefix in ("", "text_model."):
        sd = TR.clip_to_hf(w, prefix)
        sd[prefix + "embeddings.position_ids"] = torch.arange(77)[None]       # the buffer old checkpoints persist
        enc = NativeClipText.from_hf_state_dict(sd, cfg)
        _same_table(enc, w)
        assert enc.eos_token_id is None and enc.proj_dim == 0 and enc.batch_invariant
    assert NativeClipText.from_hf_state_dict(TR.clip_to_hf(w), dict(cfg, eos_token_id=300)).eos_token_id == 300
    # CLIPTextModelWithProjection: an nn.Linear [proj][width] becomes CLIP's [width][proj]
    wp = toy_weights(True)
    enc = NativeClipText.from_hf_state_dict(TR.clip_to_hf(wp), cfg)
    _same_table(enc, wp)
    assert enc.proj_dim == t["proj_dim"]


def test_transformers_own_state_dict_loads():
    """the names come from the installed transformers, not from this project's idea of them"""
    from transformers import CLIPTextConfig, CLIPTextModel
    c = CLIPTextConfig(vocab_size=64, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
                       max_position_embeddings=16, hidden_act="quick_gelu")
    m = CLIPTextModel(c)
    enc = NativeClipText.from_hf_state_dict(m.state_dict(), c)
    assert list(enc.params) == list(text_param_shapes(64, 2, 64, 16))
    own = {k.replace("text_model.", ""): v for k, v in m.state_dict().items()}
    want = torch.cat([own[f"encoder.layers.1.self_attn.{p}_proj.weight"] for p in "qkv"])
    assert torch.equal(enc.params["transformer.resblocks.1.attn.in_proj_weight"], want)


def test_openai_state_dict_ignores_the_visual_tower():
    w = toy_weights(True)
    sd = dict(w)
    sd.update({"visual.conv1.weight": torch.zeros(4, 3, 2, 2), "visual.transformer.resblocks.0.ln_1.weight": torch.zeros(4),
               "logit_scale": torch.zeros(()), "input_resolution": torch.tensor(224), "context_length": torch.tensor(77),
               "vocab_size": torch.tensor(512)})
    enc = NativeClipText.from_clip_state_dict(sd)
    _same_table(enc, w)
    t = TR.TOY
    assert (enc.width, enc.layers, enc.heads, enc.vocab_size, enc.context_length, enc.proj_dim) == (
        t["width"], t["layers"], t["heads"], t["vocab_size"], t["context_length"], t["proj_dim"])


def test_standin_maps_onto_the_same_names_and_computes_the_same_function():
    s = ClipTextEncoder(dim=64, layers=2, heads=1, vocab=96, max_len=12, seed=3)
    enc = NativeClipText.from_standin(s)
    assert list(enc.params) == list(text_param_shapes(64, 2, 96, 12))
    ids = torch.tensor([[94] + TR.word_ids(6, 5, 1, 94) + [95] * 5])
    h, _ = TR.text_forward(enc.params, ids, 1)
    assert TR.rel_l2(h, s(ids)[0]) < LIMIT


def test_checkpoint_mistakes_are_reported():
    t = TR.TOY
    w = toy_weights(False)
    cfg = dict(hidden_size=t["width"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"], vocab_size=t["vocab_size"],
               max_position_embeddings=t["context_length"], hidden_act="quick_gelu")
    sd = TR.clip_to_hf(w)
    # q / k / v order: a checkpoint with k and q exchanged does NOT give the table of the right one
    sw = dict(sd)
    sw["encoder.layers.0.self_attn.q_proj.weight"], sw["encoder.layers.0.self_attn.k_proj.weight"] = (
        sd["encoder.layers.0.self_attn.k_proj.weight"], sd["encoder.layers.0.self_attn.q_proj.weight"])
    got = NativeClipText.from_hf_state_dict(sw, cfg).params["transformer.resblocks.0.attn.in_proj_weight"]
    assert not torch.equal(got, w["transformer.resblocks.0.attn.in_proj_weight"])
    assert torch.equal(got[:128], w["transformer.resblocks.0.attn.in_proj_weight"][128:256])
    miss = {k: v for k, v in sd.items() if k != "encoder.layers.1.self_attn.v_proj.bias"}
    with pytest.raises(KeyError, match=r"missing \['transformer.resblocks.1.attn.in_proj_bias'\] \(1\), unexpected \[\] \(0\)"):
        NativeClipText.from_hf_state_dict(miss, cfg)
    with pytest.raises(KeyError, match=r"unexpected \['encoder.layers.0.rotary.weight'\] \(1\)"):
        NativeClipText.from_hf_state_dict(dict(sd, **{"encoder.layers.0.rotary.weight": torch.zeros(1)}), cfg)
    with pytest.raises(KeyError, match="unexpected"):
        NativeClipText.from_clip_state_dict(dict(toy_weights(True), extra=torch.zeros(1)))
    with pytest.raises(KeyError, match="missing"):
        NativeClipText.from_clip_state_dict({k: v for k, v in w.items() if k != "ln_final.bias"})
    bad = dict(sd)
    bad["final_layer_norm.weight"] = torch.zeros(7)
    with pytest.raises(ValueError, match="ln_final.weight: expected shape"):
        NativeClipText.from_hf_state_dict(bad, cfg)


def test_unsupported_models_are_refused_by_name():
    cfg = dict(hidden_size=1024, num_hidden_layers=23, num_attention_heads=16, vocab_size=49408, max_position_embeddings=77,
               hidden_act="gelu")
    with pytest.raises(NotImplementedError, match="'gelu'"):
        NativeClipText.from_hf_state_dict({}, cfg)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        NativeClipText.from_hf_state_dict({}, dict(cfg, hidden_act="quick_gelu", hidden_size=512))
    with pytest.raises(NotImplementedError, match="head dimension 16"):
        NativeClipText.from_standin(ClipTextEncoder(dim=64, layers=1, heads=4, vocab=8, max_len=4))
    with pytest.raises(NotImplementedError):
        NativeClipText(width=96, layers=1, heads=1, vocab_size=8, context_length=4)


def test_ids_are_validated_on_the_host_before_anything_runs():
    enc = NativeClipText.from_clip_state_dict(toy_weights(True))
    for bad in (512, -1):
        ids = torch.tensor([[510, 3, bad, 511]])
        with pytest.raises(ValueError, match=rf"token id {bad} outside \[0, 512\)"):
            enc(ids)
    with pytest.raises(ValueError, match="integer"):
        enc(torch.zeros(1, 4))
    assert enc.calls == 0 and enc._h is None


def test_pool_index_rules():
    enc = NativeClipText(64, 1, 1, 512, 8)
    ids = torch.tensor([[299, 400, 300, 300], [299, 300, 300, 300]])
    assert enc.pool_index(ids).tolist() == [1, 1]
    enc = NativeClipText(64, 1, 1, 512, 8, eos_token_id=300)
    assert enc.pool_index(ids).tolist() == [2, 1]
    assert NativeClipText(64, 1, 1, 512, 8, eos_token_id=2).eos_token_id is None      # the legacy config value: argmax


def test_text_encoder_directory_in_transformers_layout_loads(tmp_path):
    """what from_pretrained(native_text=True) does with <path>/text_encoder: config.json + model.safetensors under
    transformers' file name, `text_model.` names and the persisted position_ids buffer"""
    from safetensors.torch import save_file
    from hedit import checkpoint as CK
    t = TR.TOY
    w = toy_weights(False)
    d = tmp_path / "text_encoder"
    d.mkdir()
    sd = TR.clip_to_hf(w, "text_model.")
    sd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    cfg = dict(architectures=["CLIPTextModel"], hidden_size=t["width"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"],
               vocab_size=t["vocab_size"], max_position_embeddings=t["context_length"], hidden_act="quick_gelu", eos_token_id=2,
               intermediate_size=4 * t["width"])
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    assert CK.read_config(str(d)) == cfg
    rcfg, rsd = CK.read_component(str(d))
    enc = NativeClipText.from_hf_state_dict(rsd, rcfg)
    _same_table(enc, w)
    assert enc.eos_token_id is None and enc.context_length == 77
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        NativeClipText(64, 1, 1, 8, 4, proj_dim=6)
