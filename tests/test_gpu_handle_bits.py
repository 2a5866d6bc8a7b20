"""-m gpu: the parameter tables, the workspace sizes and the output bits of the seven handle families that
tests/golden/g23_encoder_bits.json does not cover -- unet, vae, ddpm, irse50, faceparse, lpips, sqlpips -- are pinned to
tests/golden/g27_handle_bits.json; the tables of the four transformer encoders go in as well (table only, their bits are
g23's).  Per case: the list of [name, ndim, dims] of every create variant (for the UNet with the bf16_exact flag per
entry), pinned as the row count and the SHA-256 of the rows -- a mismatch prints the rows it got; the value of every
*_workspace_bytes / *_grad_workspace_bytes entry at the case's shapes; and the SHA-256 of every
output tensor's bytes.

The golden file was written on an MI355X by the library built from the commit it names (`parent_commit`: the last one in
which csrc/unet.hip carried its own parameter store and every model file its own copy of the C-ABI lifecycle), never by the
code under test:
    HEDIT_LIB_VARIANT=parent python tests/test_gpu_handle_bits.py --write --parent <commit>
loads hedit/lib_parent.so.bin (a side library, as the tools' A/B runs do), runs every case twice and writes the JSON; a case
whose two runs disagree would go under "unstable" (none of these cases draws random numbers, so none may).  Under pytest the
product library must reproduce every table, size and hash.  Moving code between files keeps them; a change of the order or
shape of a registered parameter, of a pack launch, of arithmetic or of an arena's alloc / free sequence does not.

Weights come from each wrapper's seeded init_random; inputs are made on the CPU from a seed and copied to the device.
  unet       TINY_CONFIG at 32 x 32 latents: forward at B = 1 and B = 2, forward_shared with B = 2 rows of D = 1 latent;
             forward_keep + backward on the create_grad handle (B = 2); forward_keep + backward_ctx on the create_grad_ctx
             handle (B = 1)
  unet_chain a two-level config whose attention level has ffn_fused_channels() = 320 channels, so that the stream pack
             kinds (ffn.hip / linchain.hip) are registered, which TINY_CONFIG's widths never reach: create / create_grad,
             table + bf16_exact + missing only -- no load, no forward
  vae        TINY_VAE_CONFIG at an 8 x 8 latent, B = 2: decode, decode_vjp, encode
  ddpm       TINY_DDPM_CONFIG (32 x 32): forward and vjp at B = 1 and B = 2
  irse50     features and cos_fwd_bwd on its fixed 256 x 256 input, B = 2
  faceparse  labels at 32 x 32, B = 2
  lpips      source and fwd_bwd at 32 x 32, B = 2
  sqlpips    distance at 32 x 32, B = 2
  encoders   text / clipimg / dino / vit at the widths of tests/test_gpu_encoder_bits.py: table only
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h-edit_amd"))
from hedit import _lib  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "g27_handle_bits.json")
DEV = "cuda:0"
CASES = ("unet", "unet_chain", "vae", "ddpm", "irse50", "faceparse", "lpips", "sqlpips", "encoders")


def _sha(t):
    t = t.detach().cpu().contiguous()
    assert t.dtype == torch.int64 or torch.isfinite(t).all()
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _normal(shape, seed, scale=1.0):
    return (torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)) * scale).to(DEV)


def _image(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)).to(DEV)


TABLES = {}      # digest -> rows, of the tables this process read: printed when a table does not match


def _table(fam, h, exact=False):
    """the [name, ndim, dims(, bf16_exact)] rows of handle `h` of family `fam`, in the library's order, as their count and the
    SHA-256 of their JSON lines: a table of several hundred rows is one line of the golden file"""
    lib, nd, dims, out = _lib.lib(), C.c_int(), (C.c_int * 4)(), []
    fn = lambda what: getattr(lib, f"hedit_{fam}_{what}")  # noqa: E731
    for i in range(fn("num_params")(h)):
        _lib.check(fn("param_shape")(h, i, C.byref(nd), dims))
        row = [fn("param_name")(h, i).decode(), nd.value, list(dims)]
        out.append(json.dumps(row + [int(fn("param_bf16_exact")(h, i))] if exact else row))
    digest = hashlib.sha256("\n".join(out).encode()).hexdigest()
    TABLES[digest] = out
    return dict(rows=len(out), sha256=digest)


def _created(fam, cfg=None, create="create", exact=False):
    """table (and count of unloaded parameters) of a handle that is created and destroyed again, nothing loaded"""
    lib, h = _lib.lib(), C.c_void_p()
    _lib.check(getattr(lib, f"hedit_{fam}_{create}")(*(() if cfg is None else (C.byref(cfg),)), C.byref(h)))
    try:
        return dict(table=_table(fam, h, exact), missing=getattr(lib, f"hedit_{fam}_missing")(h))
    finally:
        getattr(lib, f"hedit_{fam}_destroy")(h)


def _unet():
    from hedit.unet import TINY_CONFIG, UNet2DConditionModel
    lib, out = _lib.lib(), {}
    D = TINY_CONFIG["cross_attention_dim"]
    m = UNet2DConditionModel(TINY_CONFIG, device=DEV)
    out["create"] = dict(table=_table("unet", m._h, True))
    m.init_random(11)
    for B in (1, 2):
        x, ctx = _normal((B, 4, 32, 32), 100 + B), _normal((B, 77, D), 110 + B)
        out[f"forward_B{B}"] = dict(workspace_bytes=lib.hedit_unet_workspace_bytes(m._h, B, 32, 32), eps=_sha(m.forward_raw(x, 500.0, ctx)))
    x, ctx = _normal((1, 4, 32, 32), 120), _normal((2, 77, D), 121)
    out["forward_shared_B2_D1"] = dict(eps=_sha(m.forward_raw(x, 500.0, ctx, row_latent=[0, 0])))
    m._native_release()

    m = UNet2DConditionModel(TINY_CONFIG, device=DEV, grad=True)
    out["create_grad"] = dict(table=_table("unet", m._h, True))
    m.init_random(11)
    x, ctx, g = _normal((2, 4, 32, 32), 130), _normal((2, 77, D), 131), _normal((2, 4, 32, 32), 132)
    need = lib.hedit_unet_grad_workspace_bytes(m._h, 2, 32, 32)
    _, eps = m._keep(x, 300.0, ctx)
    dx = torch.empty_like(x)
    _lib.check(lib.hedit_unet_backward(m._h, _lib.ptr(g), _lib.ptr(dx), _lib.ptr(m._gws), _lib.cur_stream()))
    out["keep_backward_B2"] = dict(grad_workspace_bytes=need, workspace_bytes=lib.hedit_unet_workspace_bytes(m._h, 2, 32, 32),
                                   eps=_sha(eps), d_x=_sha(dx))
    m._release()
    m._native_release()

    m = UNet2DConditionModel(TINY_CONFIG, device=DEV, grad="context")
    out["create_grad_ctx"] = dict(table=_table("unet", m._h, True))
    m.init_random(11)
    x, ctx, g = _normal((1, 4, 32, 32), 140), _normal((1, 77, D), 141), _normal((1, 4, 32, 32), 142)
    need = lib.hedit_unet_grad_workspace_bytes(m._h, 1, 32, 32)
    _, eps = m._keep(x, 300.0, ctx)
    dx, dc = torch.empty_like(x), torch.empty_like(ctx)
    _lib.check(lib.hedit_unet_backward_ctx(m._h, _lib.ptr(g), _lib.ptr(dx), _lib.ptr(dc), _lib.ptr(m._gws), _lib.cur_stream()))
    out["keep_backward_ctx_B1"] = dict(grad_workspace_bytes=need, eps=_sha(eps), d_x=_sha(dx), d_ctx=_sha(dc))
    m._release()
    m._native_release()
    return out


def _unet_chain():
    c = _lib.UnetCfg()
    c.in_channels, c.out_channels, c.sample_size, c.n_levels = 4, 4, 32, 2
    for i in range(2):
        c.block_out_channels[i] = _lib.lib().hedit_k_ffn_channels()
    c.down_has_attn[0], c.up_has_attn[1] = 1, 1
    c.layers_per_block, c.cross_attention_dim, c.heads, c.norm_num_groups = 1, 64, 8, 32
    return {v: _created("unet", c, v, True) for v in ("create", "create_grad", "create_grad_ctx")}


def _vae():
    from hedit.vae import TINY_VAE_CONFIG, AutoencoderKL
    lib, B = _lib.lib(), 2
    m = AutoencoderKL(TINY_VAE_CONFIG, device=DEV)
    out = {"create": dict(table=_table("vae", m._h))}
    m.init_random(21)
    f = m.factor
    z, d_img, img = _normal((B, 4, 8, 8), 200), _normal((B, 3, 8 * f, 8 * f), 201), _image((B, 3, 8 * f, 8 * f), 202)
    ws = {k: lib.hedit_vae_workspace_bytes(m._h, B, 8, 8, v) for k, v in (("decode", 0), ("encode", 1), ("decode_vjp", 2))}
    out["B2_8x8"] = dict(workspace_bytes=ws, decode=_sha(m.decode(z).sample), decode_vjp=_sha(m.decode_vjp(z, d_img)),
                         encode=_sha(m.encode(img).latent_dist.mode()))
    m._native_release()
    return out


def _ddpm():
    from hedit.diffusion.diffusion import TINY_DDPM_CONFIG, Model
    lib, out = _lib.lib(), {}
    m, mg = Model(TINY_DDPM_CONFIG, device=DEV), Model(TINY_DDPM_CONFIG, device=DEV, grad=True)
    out["create"], out["create_grad"] = dict(table=_table("ddpm", m._h)), dict(table=_table("ddpm", mg._h))
    m.init_random(31)
    mg.init_random(31)
    for B in (1, 2):
        x, g = _normal((B, 3, 32, 32), 300 + B), _normal((B, 3, 32, 32), 310 + B)
        need, gneed = lib.hedit_ddpm_workspace_bytes(m._h, B), lib.hedit_ddpm_grad_workspace_bytes(mg._h, B)
        ws = torch.empty(gneed, dtype=torch.uint8, device=DEV)
        dx, eps = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.hedit_ddpm_vjp(mg._h, _lib.ptr(x), 400.0, _lib.ptr(g), B, _lib.ptr(dx), _lib.ptr(eps), _lib.ptr(ws), gneed, _lib.cur_stream()))
        out[f"B{B}"] = dict(workspace_bytes=need, grad_workspace_bytes=gneed, forward=_sha(m(x, 400.0)), vjp_eps=_sha(eps), vjp_d_x=_sha(dx))
    m._native_release()
    mg._native_release()
    return out


def _irse50():
    from hedit.arcface.arcface_model import IDLoss
    B = 2
    m = IDLoss(ref=_image((1, 3, 256, 256), 400).cpu(), device=DEV, seed=41)
    x = _image((B, 3, 256, 256), 401)
    feat = m._native_features(x)
    loss, grad = m._native_loss_and_grad(x, 1.0)
    out = {"create": dict(table=_table("irse50", m._h)),
           "B2": dict(workspace_bytes=m._lib.hedit_irse50_workspace_bytes(m._h, B), features=_sha(feat), loss=_sha(loss), d_image=_sha(grad))}
    m._native_release()
    return out


def _faceparse():
    from hedit.arcface import FaceParsing
    B = 2
    m = FaceParsing(device=DEV).init_random(51).eval()
    labels = m(_image((B, 3, 32, 32), 500))
    out = {"create": dict(table=_table("faceparse", m._h)),
           "B2_32x32": dict(workspace_bytes=m._lib.hedit_faceparse_workspace_bytes(m._h, B, 32, 32), labels=_sha(labels))}
    m._native_release()
    return out


def _lpips():
    from hedit.arcface.lpips_loss import LPIPS_Loss
    B = 2
    m = LPIPS_Loss(src=_image((1, 3, 32, 32), 600).cpu(), device=DEV, seed=61)
    loss, grad = m._native_loss_and_grad(_image((B, 3, 32, 32), 601))
    out = {"create": dict(table=_table("lpips", m._h)),
           "B2_32x32": dict(workspace_bytes=m._lib.hedit_lpips_workspace_bytes(m._h, B, 32, 32), source=_sha(m._src_feats[1]), loss=_sha(loss),
                            d_x=_sha(grad))}
    m._native_release()
    return out


def _sqlpips():
    from hedit.lpips_score import NativeSqueezeLpips
    B = 2
    m = NativeSqueezeLpips(device=DEV, seed=71)
    d = m.distance(_image((B, 3, 32, 32), 700), _image((B, 3, 32, 32), 701))
    out = {"create": dict(table=_table("sqlpips", m._h)),
           "B2_32x32": dict(workspace_bytes=m._lib.hedit_sqlpips_workspace_bytes(m._h, B, 32, 32), distance=_sha(d))}
    m._native_release()
    return out


def _encoders():
    W, HEADS, LAYERS = 128, 2, 2
    return {"text": _created("text", _lib.TextCfg(W, LAYERS, HEADS, 64, 77, 64)),
            "clipimg": _created("clipimg", _lib.ClipImgCfg(W, LAYERS, HEADS, 8, 32, 64)),
            "dino": _created("dino", _lib.DinoCfg(W, 3, HEADS, 8, 96, 2)),
            "vit": _created("vit", _lib.VitCfg(W, LAYERS, HEADS, 8, 32))}


def run_case(name):
    with torch.no_grad():
        out = globals()["_" + name]()
    torch.cuda.synchronize()
    return json.loads(json.dumps(out))      # tuples -> lists, as the golden file reads back


@pytest.mark.parametrize("name", CASES)
def test_handle_tables_workspaces_and_bits_match_the_parent_commit(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    doc = json.load(open(GOLDEN))
    assert name in doc["cases"] and not doc["unstable"], (name, list(doc["unstable"]))
    want, got = doc["cases"][name], run_case(name)
    for call, rec in got.items():
        print(f"[handle bits] {name} {call}: " + ", ".join(f"{k} {v['rows'] if k == 'table' else str(v)[:12]}" for k, v in rec.items()))
        if "table" in rec and rec["table"] != want[call]["table"]:
            print("\n".join(TABLES[rec["table"]["sha256"]]))
        assert rec == want[call], (name, call, rec, want[call])
    assert got.keys() == want.keys()


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: [HEDIT_LIB_VARIANT=NAME] python tests/test_gpu_handle_bits.py --write [--parent COMMIT] [--out FILE]")
    if os.environ.get("HEDIT_LIB_VARIANT"):        # a side library hedit/lib_NAME.so.bin, as the tools' A/B runs load it
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"lib_{os.environ['HEDIT_LIB_VARIANT']}.so.bin")
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else "unknown"
    ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()
    doc = dict(parent_commit=parent, library=os.path.basename(_lib.LIB_PATH), hipcc=ver[0] if ver else "unknown", cases={}, unstable={})
    for name in CASES:
        a, b = run_case(name), run_case(name)
        doc["cases" if a == b else "unstable"][name] = a if a == b else [a, b]
        print(name, "stable" if a == b else "UNSTABLE", flush=True)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from", _lib.LIB_PATH)
