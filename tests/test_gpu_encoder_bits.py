"""-m gpu: the output bits and the workspace sizes of the four transformer encoders (hedit_text_*, hedit_clipimg_*,
hedit_dino_*, hedit_vit_* of csrc/text.hip, clipimg.hip, dino.hip, vit.hip on the shared kernels and block driver of
csrc/encoder.hip / encoder.h) are pinned to tests/golden/g23_encoder_bits.json: per case the SHA-256 of every output
tensor's bytes and the value of the handle's *_workspace_bytes.

The golden file was written on an MI355X by the library built from the commit it names (`parent_commit`: the last one in
which every encoder file carried its own copy of these kernels), never by the code under test:
    HEDIT_LIB_VARIANT=parent python tests/test_gpu_encoder_bits.py --write --parent <commit>
loads hedit/lib_parent.so.bin (a side library, as the tools' A/B runs do) and writes the JSON; under pytest the product
library must reproduce every hash and every size.  Moving code between files, or a change of parameterisation, keeps them;
any change of arithmetic, of summation order or of the arena's alloc / free sequence does not.

All cases: width 128, 2 heads, 2 whole blocks, the default (bf16) storage build; the outputs are fp32 and do not depend on
the storage build (the "other storage build" tests of the four encoders' own files).  Weights are the seeded stand-ins of
tests/helpers/text_ref.py, clipimg_ref.py, hedit.dino_score.DinoNet.init_random and ClipVisualPrefix.init_random; inputs are
made on the CPU from a seed and copied to the device: no torch GPU arithmetic sits between a seed and a native call.
  text     vocab 64, context 77, proj_dim 0 and 64; B = 3 at L = 77 (more rows than waves: the boustrophedon deal runs) and
           B = 1 at L = 9; hidden and pooled (the transposed weight packing, the row gather with an index)
  clipimg  patch 8, embed_dim 64; R = 32 (17 tokens, one ragged tile) and R = 96 (145 tokens: two key tiles, five passes);
           B = 2 (the row gather without an index)
  dino     patch 8, R = 96; three layers with key_layer 2, and key_layer 0; S = 96 (copy) and S = 160 (resize); keys with
           B = 2 and structure_distance with N = 2 (tokens with the conv bias, bias without residual, eps 1e-6)
  vit      patch 8; R = 32 (17 tokens) and R = 112 (197 tokens, the production count); B = 2; hedit_vit_gram and
           hedit_vit_gram_fwd_bwd (LayerNorm with statistics, patchify backward, forward + input-gradient weight packing)
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

GOLDEN = os.path.join(HERE, "golden", "g23_encoder_bits.json")
DEV = "cuda:0"
W, HEADS, LAYERS = 128, 2, 2

CASES = ("text_p0", "text_p64", "clipimg_r32", "clipimg_r96", "dino_k2_s96", "dino_k2_s160", "dino_k0_s96", "dino_k0_s160", "vit_r32", "vit_r112")


def _sha(t):
    t = t.detach().cpu().contiguous()
    assert torch.isfinite(t).all()
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _normal(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


class _Handle:
    """a native handle of family `fam`, created from `cfg` and loaded from the CPU state dict `sd`"""

    def __init__(self, fam, cfg, sd):
        self.lib, self.fam = _lib.lib(), fam
        self.h = C.c_void_p()
        _lib.check(self.fn("create")(C.byref(cfg), C.byref(self.h)))
        try:
            for i in range(self.fn("num_params")(self.h)):
                name = self.fn("param_name")(self.h, i).decode()
                w = sd[name].detach().to(torch.float32).contiguous().to(DEV)
                _lib.check(self.fn("load")(self.h, name.encode(), _lib.ptr(w), w.numel(), _lib.cur_stream()))
                torch.cuda.current_stream().synchronize()
            _lib.check(self.fn("finalize")(self.h, _lib.cur_stream()))
        except Exception:
            self.close()
            raise

    def fn(self, what):
        return getattr(self.lib, f"hedit_{self.fam}_{what}")

    def close(self):
        if self.h is not None:
            self.fn("destroy")(self.h)
            self.h = None


def _ws(nbytes):
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)


def _text(proj):
    from helpers.text_ref import text_weights
    cfg = dict(width=W, layers=LAYERS, heads=HEADS, vocab_size=64, context_length=77, proj_dim=proj)
    h = _Handle("text", _lib.TextCfg(*cfg.values()), text_weights(**cfg))
    out = {}
    try:
        for B, L in ((3, 77), (1, 9)):
            g = np.random.default_rng(1000 + 10 * B + L)
            ids = torch.from_numpy(g.integers(0, 64, (B, L)).astype(np.int32)).to(DEV)
            pidx = torch.from_numpy(g.integers(0, L, (B,)).astype(np.int32)).to(DEV)
            hidden = torch.empty(B, L, W, device=DEV)
            pooled = torch.empty(B, proj or W, device=DEV)
            need = h.fn("workspace_bytes")(h.h, B, L)
            ws = _ws(need)
            _lib.check(h.fn("encode")(h.h, _lib.ptr(ids), B, L, _lib.ptr(hidden), _lib.ptr(pidx), _lib.ptr(pooled), _lib.ptr(ws), need, _lib.cur_stream()))
            out[f"B{B}_L{L}"] = dict(workspace_bytes=need, hidden=_sha(hidden), pooled=_sha(pooled))
    finally:
        h.close()
    return out


def _clipimg(R):
    from helpers.clipimg_ref import clipimg_weights, test_images
    cfg = dict(width=W, layers=LAYERS, heads=HEADS, patch_size=8, input_resolution=R, embed_dim=64)
    h = _Handle("clipimg", _lib.ClipImgCfg(*cfg.values()), clipimg_weights(**cfg))
    try:
        B = 2
        img = test_images(B, R, 2000 + R).to(DEV)
        o = torch.empty(B, 64, device=DEV)
        need = h.fn("workspace_bytes")(h.h, B)
        ws = _ws(need)
        _lib.check(h.fn("encode")(h.h, _lib.ptr(img), B, _lib.ptr(o), _lib.ptr(ws), need, _lib.cur_stream()))
        return {"B2": dict(workspace_bytes=need, out=_sha(o))}
    finally:
        h.close()


def _dino(key_layer, S):
    from hedit.dino_score import DinoNet
    R, N = 96, 2
    net = DinoNet(W, 3, 8, R, key_layer).init_random(3000 + key_layer)
    h = _Handle("dino", _lib.DinoCfg(W, 3, HEADS, 8, R, key_layer), net.params)
    try:
        g = np.random.default_rng(3100 + S)
        a = torch.from_numpy(g.uniform(0, 255, (N, 3, S, S)).astype(np.float32)).to(DEV)
        b = torch.from_numpy(g.uniform(0, 255, (N, 3, S, S)).astype(np.float32)).to(DEV)
        L = (R // 8) ** 2 + 1
        keys = torch.empty(2, L, W, device=DEV)
        dist = torch.empty(N, device=DEV)
        need = h.fn("workspace_bytes")(h.h, N, S)
        ws = _ws(need)
        _lib.check(h.fn("keys")(h.h, _lib.ptr(a), 2, S, _lib.ptr(keys), _lib.ptr(ws), need, _lib.cur_stream()))
        _lib.check(h.fn("structure_distance")(h.h, _lib.ptr(a), _lib.ptr(b), N, S, _lib.ptr(dist), _lib.ptr(ws), need, _lib.cur_stream()))
        return {"N2": dict(workspace_bytes=need, keys=_sha(keys), dist=_sha(dist))}
    finally:
        h.close()


def _vit(R):
    from hedit.clip_guidance.base_clip import ClipVisualPrefix
    net = ClipVisualPrefix(W, LAYERS, HEADS, 8, R).init_random(4000 + R)
    h = _Handle("vit", _lib.VitCfg(W, LAYERS, HEADS, 8, R), net.state_dict())
    try:
        B = 2
        img = _normal((B, 3, R, R), 4100 + R).to(DEV)
        gref = _normal((W, W), 4200 + R).to(DEV)
        gram = torch.empty(B, W, W, device=DEV)
        loss = torch.empty(B, device=DEV)
        d_img = torch.empty(B, 3, R, R, device=DEV)
        need = h.fn("workspace_bytes")(h.h, B)
        ws = _ws(need)
        _lib.check(h.fn("gram")(h.h, _lib.ptr(img), B, _lib.ptr(gram), _lib.ptr(ws), need, _lib.cur_stream()))
        _lib.check(h.fn("gram_fwd_bwd")(h.h, _lib.ptr(img), _lib.ptr(gref), 0, B, 1.0, _lib.ptr(loss), _lib.ptr(d_img), _lib.ptr(ws), need,
                                        _lib.cur_stream()))
        return {"B2": dict(workspace_bytes=need, gram=_sha(gram), loss=_sha(loss), d_image=_sha(d_img))}
    finally:
        h.close()


def run_case(name):
    fam, *arg = name.split("_")
    if fam == "text":
        return _text(int(arg[0][1:]))
    if fam == "clipimg":
        return _clipimg(int(arg[0][1:]))
    if fam == "dino":
        return _dino(int(arg[0][1:]), int(arg[1][1:]))
    return _vit(int(arg[0][1:]))


@pytest.mark.parametrize("name", CASES)
def test_encoder_bits_and_workspace_match_the_parent_commit(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    want = json.load(open(GOLDEN))["cases"][name]
    got = run_case(name)
    for call, rec in got.items():
        print(f"[encoder bits] {name} {call}: " + ", ".join(f"{k} {str(v)[:12]}" for k, v in rec.items()))
    assert got == want, (name, got, want)


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: [HEDIT_LIB_VARIANT=NAME] python tests/test_gpu_encoder_bits.py --write [--parent COMMIT] [--out FILE]")
    if os.environ.get("HEDIT_LIB_VARIANT"):        # a side library hedit/lib_NAME.so.bin, as the tools' A/B runs load it
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"lib_{os.environ['HEDIT_LIB_VARIANT']}.so.bin")
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else "unknown"
    ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()
    doc = dict(parent_commit=parent, library=os.path.basename(_lib.LIB_PATH), hipcc=ver[0] if ver else "unknown",
               cases={name: run_case(name) for name in CASES})
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from", _lib.LIB_PATH)
