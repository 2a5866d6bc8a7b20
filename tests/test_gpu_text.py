"""-m gpu: the native prompt encoder (hedit_text_* of csrc/text.hip on the shared encoder kernels and block forward of
csrc/encoder.hip / encoder.h, behind hedit.text.NativeClipText; SURVEY.md section 8
row a7) against tests/golden/g19_text.npz -- vectors recorded by RUNNING the reference's ``CLIP.encode_text`` and
transformers' CLIPTextModel (tests/golden/make_golden_text.py; pinned on the host by tests/test_host_text.py).

Limit of every comparison with a reference: 1e-4 relative L2, the project's limit for this GEMM class (fp32 stream,
three-term split-bf16 operands, fp32 accumulation; tests/test_gpu_clip.py).  The consumer rounds the context to its storage
type, half an ulp of which is 2^-9 = 2.0e-3 (bfloat16) or 2^-12 = 2.4e-4 (half).  Batch invariance and the prefix
property are bit for bit.

MEASURED (MI355X, bfloat16 build; relative L2, every test prints its figures with -s before it asserts):
  reference CLIP, 3 layers: hidden 8.8e-6, pooled x text_projection 1.2e-5
  transformers, 3 layers (fp64): hidden 8.9e-6, pooled 9.8e-6 (argmax rule) / 1.0e-5 (first-EOS rule)
  SD width, 12 layers (fp64): hidden 9.7e-6, pooled 9.9e-6 -- depth does not add to it; a tenth of the limit
  torch stand-in on the same GPU, 49408 tokens: 1.17e-5 (L = 77), 1.23e-5 (L = 16)
The fp32 restatement on the host is 4.0e-7 ... 7.0e-7 from the same vectors (tests/test_host_text.py).
  tiny P2P loop, native context, against the oracle: recon 3.0e-3, edit 2.3e-2 (limits 1.5e-2 / 7e-2)
Under HEDIT_STORAGE=f16 the file passes with the SAME parity figures digit for digit (the encoder does not read the storage
type); the loop: recon 3.8e-4, edit 2.9e-3.  Wall time of the file: 10 s in either build (8.6 s / 7.5 s inside pytest).
"""
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
from helpers import text_ref as TR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.text import ClipTextEncoder, NativeClipText, text_param_shapes  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 1e-4


@pytest.fixture(scope="module")
def gold():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(os.path.join(GOLD, "g19_text.npz")), json.load(open(os.path.join(GOLD, "g19_text.json")))


@pytest.fixture(scope="module")
def sd_enc(gold):
    """SD-1.x width, 12 layers, 1024-row vocabulary: the fixture's weights, regenerated from their names"""
    t = TR.SDW
    w = TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], 0)
    return NativeClipText.from_clip_state_dict(w, device=G.dev())


def _report(name, got, want):
    err = G.rel_err(got, torch.from_numpy(np.asarray(want)))
    print(f"[text parity] {name}: rel L2 {err:.3e}")
    return err


def test_parity_with_the_reference_clip(gold):
    g, meta = gold
    t = TR.TOY
    w = TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"])
    enc = NativeClipText.from_clip_state_dict(w, device=G.dev())
    out = enc(torch.tensor(meta["ref_ids"]))
    G.sync()
    assert out[0].shape == (3, 77, 128) and out[1].shape == (3, 32) and out[0].dtype == torch.float32 and out[0].is_cuda
    errs = [_report("reference hidden (3 layers)", out[0], g["ref_hidden"]), _report("reference pooled x text_projection", out[1], g["ref_pooled"])]
    assert max(errs) < LIMIT, errs
    # the C table is the Python table: names, order, shapes
    lib, h = _lib.lib(), enc._h
    want = text_param_shapes(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"])
    assert lib.hedit_text_num_params(h) == len(want) and lib.hedit_text_missing(h) == 0
    nd, dims = C.c_int(), (C.c_int * 4)()
    for i, (name, shape) in enumerate(want.items()):
        assert lib.hedit_text_param_name(h, i).decode() == name
        _lib.check(lib.hedit_text_param_shape(h, i, C.byref(nd), dims))
        assert tuple(dims[:nd.value]) == shape, name


def test_parity_with_transformers_under_both_pooling_rules(gold):
    g, meta = gold
    t = TR.TOY
    w = TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], 0)
    ids = torch.tensor(meta["hf_ids"])
    cfg = dict(hidden_size=t["width"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"], vocab_size=t["vocab_size"],
               max_position_embeddings=t["context_length"], hidden_act="quick_gelu")
    errs = []
    for tag, eos in (("hfa", 2), ("hfe", meta["hf_eos"])):
        enc = NativeClipText.from_hf_state_dict(TR.clip_to_hf(w, "text_model." if eos == 2 else ""), dict(cfg, eos_token_id=eos), device=G.dev())
        out = enc(ids.to(G.dev()))
        G.sync()
        errs += [_report(f"transformers hidden, eos_token_id {eos}", out[0], g["hf_hidden"]),
                 _report(f"transformers pooled, eos_token_id {eos}", out[1], g[f"{tag}_pooled"])]
    assert max(errs) < LIMIT, errs


def test_parity_at_sd_width_through_twelve_layers(gold, sd_enc):
    g, meta = gold
    out = sd_enc(torch.tensor(meta["sd_ids"]))
    G.sync()
    errs = [_report("SD width hidden (12 layers, vs fp64)", out[0], g["sd_hidden"]), _report("SD width pooled (vs fp64)", out[1], g["sd_pooled"])]
    assert max(errs) < LIMIT, errs


def _prompts(meta, n, seed0):
    V = TR.SDW["vocab_size"]
    rows = []
    for i in range(n):
        k = (3, 20, 75, 0, 41)[i % 5]
        rows.append([V - 2] + TR.word_ids(k, seed0 + i, 1, V - 2) + [V - 1] * (76 - k))
    return torch.tensor(rows)


def test_batch_invariance_bit_for_bit(gold, sd_enc):
    ids = _prompts(gold[1], 5, 50)
    a = sd_enc(ids)
    b = sd_enc(ids)
    singles = [sd_enc(ids[i:i + 1]) for i in range(5)]
    G.sync()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], torch.cat([s[0] for s in singles])) and torch.equal(a[1], torch.cat([s[1] for s in singles]))
    assert torch.isfinite(a[0]).all() and a[0].std() > 0.1


def test_prefix_property_bit_for_bit(gold, sd_enc):
    """position i depends on the tokens 0..i alone: masked keys are not read (a kernel that adds -inf and sums every key
    passes parity and fails here)"""
    ids = _prompts(gold[1], 3, 60)
    base = sd_enc(ids)[0]
    other = torch.tensor([TR.word_ids(77, 70 + b, 1, TR.SDW["vocab_size"] - 2) for b in range(3)])      # never BOS / EOS
    for p in (0, 1, 7, 40, 63, 64, 75):
        mod = ids.clone()
        mod[:, p + 1:] = other[:, p + 1:]
        assert not torch.equal(mod, ids)
        got = sd_enc(mod)[0]
        G.sync()
        assert torch.equal(got[:, :p + 1], base[:, :p + 1]), p
        assert not torch.equal(got[:, p + 1:], base[:, p + 1:]), p


def test_against_the_torch_standin_at_full_vocabulary():
    """what the product does today: the stand-in module on PyTorch-ROCm in fp32, same GPU, SD shape, 49408 tokens"""
    s = ClipTextEncoder(seed=7).to(G.dev())
    enc = NativeClipText.from_standin(s)
    tok_ids = torch.tensor([[49406] + TR.word_ids(9, 80, 1, 49406) + [49407] * 67, [49406] + TR.word_ids(75, 81, 1, 49406) + [49407]])
    errs = []
    for L in (77, 16):
        ids = tok_ids[:, :L].contiguous().to(G.dev())
        with torch.no_grad():
            want = s(ids)[0]
        out = enc(ids)
        G.sync()
        assert out[0].shape == (2, L, 768)
        errs.append(G.rel_err(out[0], want))
        print(f"[text parity] torch stand-in, full vocabulary, L = {L}: rel L2 {errs[-1]:.3e}")
        assert torch.equal(out[1], out[0][torch.arange(2), ids.argmax(-1).cpu()])      # no projection: the pooled row IS the hidden row
    assert max(errs) < LIMIT, errs


def test_engine_encodes_all_prompts_in_one_native_call():
    from hedit.engine import HEditEngine
    from hedit.pipeline import HEditPipeline
    from hedit.unet import TINY_CONFIG
    model = HEditPipeline.from_random(TINY_CONFIG, seed=0, device=G.dev(), text_layers=2, native_text=True)
    enc = model.text_encoder
    assert isinstance(enc, NativeClipText) and enc.heads == 1 and enc.width == TINY_CONFIG["cross_attention_dim"]
    eng = HEditEngine(model)
    prompts = ["", "a cat sitting on a bench", "a dog sitting on a bench", "a tall tree", "a [red] car"]
    n0 = enc.calls
    got = eng.encode(prompts)
    assert enc.calls == n0 + 1
    assert got.shape == (5, 77, enc.width) and got.dtype == torch.float32
    for i, p in enumerate(prompts):
        assert torch.equal(eng.encode([p])[0], got[i]), p
    assert enc.calls == n0 + 6
    with pytest.raises(ValueError, match="multiple of the head dimension"):
        HEditPipeline.from_random(dict(TINY_CONFIG, cross_attention_dim=96), device=G.dev(), text_layers=1, native_text=True)
    # without the flag the stand-in is built as before (four heads at the tiny width) and encoded prompt by prompt
    plain = HEditPipeline.from_random(TINY_CONFIG, seed=0, device=G.dev(), text_layers=2)
    assert isinstance(plain.text_encoder, ClipTextEncoder) and plain.text_encoder.heads == 4


def test_p2p_loop_with_the_native_encoder_matches_the_oracle():
    """h_Edit_p2p_implicit on the tiny network, prompts through the native encoder, against the oracle loop fed by the same
    stand-in weights run by torch (one head: head dimension 64).  Limits: those of tests/test_gpu_loops.py for this loop."""
    from helpers.models import make_pair
    from helpers.tiny import PROMPT_PAIRS
    from hedit.inversion import p2p_h_edit as HE
    from hedit.unet import TINY_CONFIG
    from oracle import loops as OL
    from test_gpu_loops import controllers, tol
    T, after = 8, 4          # CASES[0] of tests/test_gpu_loops.py with its own set-up (seeds, T = 8, the last 4 steps, K = 1): what its limit was taken on
    hip, om, _ = make_pair(TINY_CONFIG, T, out_scale=0.3)
    standin = ClipTextEncoder(dim=TINY_CONFIG["cross_attention_dim"], layers=2, heads=1, seed=7)
    om.text_encoder = standin
    hip.text_encoder = NativeClipText.from_standin(standin, device=G.dev())
    torch.manual_seed(11)
    w0 = torch.randn(1, 4, 32, 32) * 0.8
    torch.manual_seed(100)
    src, tar = PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]
    zs, wts, _ = OL.ddpm_inversion(om, w0, eta=1.0, prompt=src, cfg_src=1.0, T=T)
    hc, oc = controllers(hip, om, 0, after, True)
    kw = dict(eta=1.0, prompts=[src, tar], cfg_scales=[1.0, 5.0, 7.5], after_skip_steps=after, is_ddim_inversion=False,
              weight_reconstruction=0.1, optimization_steps=1)
    with torch.no_grad():
        e_o, r_o = OL.h_edit_p2p_implicit(om, xT=wts[after], zs=zs[:after], controller=oc, **kw)
    n0 = hip.text_encoder.calls
    e_h, r_h = HE.h_Edit_p2p_implicit(hip, xT=G.f32(wts[after]), zs=G.f32(zs[:after]), controller=hc, prog_bar=False, **kw)
    G.sync()
    assert hip.text_encoder.calls > n0 and torch.isfinite(e_h).all()
    tol_edit, tol_recon = tol(after)
    errs = (G.rel_err(r_h, r_o), G.rel_err(e_h, e_o), G.rel_err(r_h, w0))
    print(f"[text loop] recon vs oracle {errs[0]:.3e}, edit vs oracle {errs[1]:.3e}, recon vs w0 {errs[2]:.3e} (limits {tol_recon}, {tol_edit}, {tol_recon})")
    G.within(errs[0], tol_recon)
    G.within(errs[1], tol_edit)
    G.within(errs[2], tol_recon)


def test_driver_with_native_text_writes_images_and_batches_identically(tmp_path):
    from PIL import Image
    from test_gpu_driver import _dataset, _driver
    d = _dataset(tmp_path)
    common = ["--data_path", str(d), "--random_init", "--tiny", "--native_text", "--num_diffusion_steps", "4", "--edit_category_list", "0", "1",
              "--mode", "h_edit_D_p2p", "--eta", "0.0", "--implicit", "--optimization_steps", "2"]
    one = _driver().main(common + ["--output_path", str(tmp_path / "r1")])
    two = _driver().main(common + ["--output_path", str(tmp_path / "r2"), "--batch", "2"])
    assert len(one) == len(two) == 2
    for a, b in zip(sorted(one), sorted(two)):
        assert os.path.basename(a) == os.path.basename(b)
        im = np.array(Image.open(a))
        assert im.shape == (256, 256, 3) and im.std() > 0
        assert np.array_equal(im, np.array(Image.open(b)))


def test_errors_are_reported_before_anything_is_launched(gold):
    t = TR.TOY
    w = TR.text_weights(t["width"], t["layers"], t["vocab_size"], t["context_length"], t["proj_dim"])
    enc = NativeClipText.from_clip_state_dict(w, device=G.dev())
    ok = enc(torch.tensor(gold[1]["ref_ids"]))[0].clone()
    n0 = enc.calls
    with pytest.raises(ValueError, match=r"token id 512 outside \[0, 512\)"):
        enc(torch.tensor([[510, 512, 511]]))
    with pytest.raises(_lib.HipError, match="context_length"):
        enc(torch.zeros(1, 78, dtype=torch.int64))
    assert enc.calls == n0
    lib, h, dev = _lib.lib(), enc._h, G.dev()
    B, L = 2, 77
    ids = torch.tensor(gold[1]["ref_ids"][:B], dtype=torch.int32, device=dev)
    pidx = torch.zeros(B, dtype=torch.int32, device=dev)
    hidden = torch.full((B, L, t["width"]), -7.0, device=dev)
    pooled = torch.full((B, t["proj_dim"]), -7.0, device=dev)
    need = lib.hedit_text_workspace_bytes(h, B, L)
    assert need > 0 and lib.hedit_text_workspace_bytes(h, B, 78) == 0 and lib.hedit_text_workspace_bytes(h, 0, L) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(B=B, L=L, hid=hidden, pi=pidx, po=pooled, nbytes=need):
        return lib.hedit_text_encode(h, _lib.ptr(ids), B, L, _lib.ptr(hid), _lib.ptr(pi), _lib.ptr(po), _lib.ptr(ws), nbytes, _lib.cur_stream())

    for kw, msg in ((dict(L=78), "context_length"), (dict(L=0), "context_length"), (dict(B=0), "B >= 1"),
                    (dict(nbytes=need // 2), "workspace too small"), (dict(pi=None), "pooled needs pool_index"),
                    (dict(hid=None, po=None), "nothing to write")):
        rc = call(**kw)                                                 # the message is that of the LAST failed call: read it right away
        assert rc == -1 and msg in lib.hedit_last_error().decode(), (kw, rc, msg, lib.hedit_last_error())
    G.sync()
    assert (hidden == -7.0).all() and (pooled == -7.0).all()          # nothing ran
    assert call() == 0
    assert call(po=None, pi=None) == 0                                  # hidden alone needs no pool_index
    G.sync()
    assert torch.equal(hidden, ok[:B])
    cfg = _lib.TextCfg(96, 1, 1, 8, 4, 0)
    hh = C.c_void_p()
    assert lib.hedit_text_create(C.byref(cfg), C.byref(hh)) == -1 and "head dimension" in lib.hedit_last_error().decode()
    cfg = _lib.TextCfg(64, 1, 1, 8, 201, 0)
    assert lib.hedit_text_create(C.byref(cfg), C.byref(hh)) == -1 and "200" in lib.hedit_last_error().decode()
    cfg = _lib.TextCfg(64, 0, 1, 8, 4, 0)
    assert lib.hedit_text_create(C.byref(cfg), C.byref(hh)) == -1 and "positive" in lib.hedit_last_error().decode()
