"""-m gpu: the kernels that the SD UNet's input-gradient pass adds to the decoder's and the pixel UNet's (csrc/attnbwd.hip,
layernorm_bwd / geglu_bwd of csrc/grad.hip, the padding-1 form of csrc/s2dgrad.hip), one by one through the C ABI against
fp64 torch.autograd on the operands after their rounding to the storage format; then the executor built from them
(csrc/unetgrad.h: hedit_unet_forward_keep / _backward / _vjp on a handle from hedit_unet_create_grad) and its autograd facade
(hedit.unet.UNet2DConditionModel(grad=True)) against torch.autograd on the fp32 CPU oracle (oracle/sd_unet.py).

Tolerances (relative L2, through G.within: half storage gets a quarter):

* attention backward, 6e-3 for each of dq, dk, dv: the project's conv-dgrad limit (tests/test_gpu_grad_kernels.py).  An fp64
  emulation of the kernel's roundings (P, dS and O rounded to bfloat16 before their products, everything else exact) gave
  1.6e-3 .. 2.0e-3 at six of the shapes below, so the limit is about three times the rounding floor.
* layernorm_bwd / geglu_bwd, 5e-3: one 16-bit rounding of the output after fp32 arithmetic, what the GroupNorm backward
  gets in tests/test_gpu_grad_kernels.py.
* padding-1 stride-2 conv input gradient, 6e-3 on the whole tensor and on each border, as its (0,1,0,1) twin in
  tests/test_gpu_ddpm_grad.py, on that file's shapes.

* whole-network VJP, 4e-2: the project's limit for whole-network VJPs from these kernels (tests/test_gpu_vae.py,
  tests/test_gpu_ddpm_grad.py).  For scale, measured on the CPU: bf16 autocast of the oracle moves its own VJP by 2.5e-2 on
  TINY_CONFIG at both sizes and by 1.9e-2 on a 320 / 160-wide variant; bf16 rounding of the residual stream alone moves it by
  1.3e-2.  Linearity in the cotangent: 2e-2 (tests/test_gpu_vae.py).  The taped eps: TOL_TINY of tests/test_gpu_unet.py.

The executor's shapes are 32 x 32 latents throughout: every configuration here has three levels and an attention in its mid
block, whose token count (H / 4)^2 must be a multiple of 64 for the forward's attention kernel -- a 16 x 16 latent (16 tokens
there) is refused by hedit_unet_forward and hedit_unet_forward_keep alike.  Token counts 1024 / 256 / 64.

What moves bits only (batch independence, repeated backward passes, the facade) is compared with torch.equal."""
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers.tiny import hash_normal  # noqa: E402
from hedit import _lib  # noqa: E402
from test_gpu_ddpm_grad import S2_SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
CTX, CTXP = 77, 80
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def dt():
    return _lib.storage_dtype()


def st(t):
    """rounded to the storage format, back in fp32 on the host"""
    return t.to(dt()).float()


def at(t, elems):
    """device pointer `elems` storage elements into t"""
    return C.c_void_p(t.data_ptr() + 2 * elems)


# ---------------------------------------------------------------------------------------------- attention backward
@functools.lru_cache(maxsize=None)
def attn_case(B, heads, N, d, keys=None):
    """q' (pre-scaled), k, v, dO rounded to storage, O = softmax(ln2 q'k^T) v in fp64 rounded to storage, and the fp64
    autograd gradients.  keys = None: self-attention (N keys); else that many context rows per image."""
    M = N if keys is None else keys
    C_ = heads * d
    seed = 1000 * d + N + 7 * B + heads
    q = st(hash_normal((B, N, C_), seed) * (d ** -0.5 * LOG2E))
    k = st(hash_normal((B, M, C_), seed + 1))
    v = st(hash_normal((B, M, C_), seed + 2))
    do = st(hash_normal((B, N, C_), seed + 3))

    def heads_of(t, n):
        return t.double().reshape(B, n, heads, d).permute(0, 2, 1, 3)

    qd, kd, vd = (heads_of(t, n).clone().requires_grad_(True) for t, n in ((q, N), (k, M), (v, M)))
    p = torch.softmax(math.log(2.0) * (qd @ kd.transpose(-1, -2)), dim=-1)
    o = p @ vd
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), heads_of(do, N))
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, C_)          # noqa: E731
    return dict(q=q, k=k, v=v, do=do, o=st(back(o.detach(), N).float()), dq=back(dq, N), dk=back(dk, M), dv=back(dv, M))


def run_self(lib, c, B, heads, N, d, interleaved, rows=None):
    """hedit_k_attn_bwd on the images `rows` of a case; interleaved: q | k share one [B*N][2C] buffer (the forward's)"""
    C_ = heads * d
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    q, k, v, o, do = (sel(c[n]) for n in ("q", "k", "v", "o", "do"))
    Bn = q.shape[0]
    if interleaved:
        qk = G.bf(torch.cat((q, k), dim=-1).reshape(Bn * N, 2 * C_))
        qp, kp, ld = _lib.ptr(qk), at(qk, C_), 2 * C_
    else:
        qd, kd = G.bf(q.reshape(Bn * N, C_)), G.bf(k.reshape(Bn * N, C_))
        qp, kp, ld = _lib.ptr(qd), _lib.ptr(kd), C_
    vd, od, dod = (G.bf(t.reshape(Bn * N, C_)) for t in (v, o, do))
    dq, dk, dv = (torch.full((Bn * N, C_), float("nan"), dtype=dt(), device=G.dev()) for _ in range(3))
    ws = torch.empty(max(lib.hedit_k_attn_bwd_ws_bytes(Bn, N, heads), 16), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_k_attn_bwd(qp, ld, kp, ld, _lib.ptr(vd), C_, _lib.ptr(od), C_, _lib.ptr(dod), C_, _lib.ptr(dq), C_,
                                    _lib.ptr(dk), _lib.ptr(dv), Bn, N, heads, d, _lib.ptr(ws), None))
    G.sync()
    return tuple(t.reshape(Bn, N, C_) for t in (dq, dk, dv))


# (B, heads, N, d, q | k interleaved): one tile; pad 40 -> 48 with head and batch offsets; d = 64; an odd tile count; d = 160;
# SD's 32 x 32 level; the tile loop at the full length of the 64 x 64 level
SELF_SHAPES = [(1, 1, 64, 32, False), (2, 2, 128, 40, True), (1, 2, 256, 64, False), (2, 1, 192, 80, True), (1, 2, 64, 160, False),
               (1, 8, 1024, 40, True), (1, 1, 4096, 40, False)]


@pytest.mark.parametrize("B,heads,N,d,interleaved", SELF_SHAPES)
def test_attn_bwd_matches_fp64_autograd(lib, B, heads, N, d, interleaved):
    c = attn_case(B, heads, N, d)
    got = run_self(lib, c, B, heads, N, d, interleaved)
    for name, g in zip(("dq", "dk", "dv"), got):
        assert torch.isfinite(g.float()).all(), name
        err = G.rel_err(g, c[name])
        print(f"attn_bwd B={B} heads={heads} N={N} d={d} {name}: {err:.3e}")
        G.within(err, 6e-3, what="attn_bwd " + name)


def run_cross(lib, c, B, heads, N, d, rows=None):
    C_ = heads * d
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    q, k, v, o, do = (sel(c[n]) for n in ("q", "k", "v", "o", "do"))
    Bn = q.shape[0]

    def padded(t):                        # [Bn][77][C] -> [Bn*80][C], the pad rows NaN: never read
        out = torch.full((Bn, CTXP, C_), float("nan"))
        out[:, :CTX] = t
        return G.bf(out.reshape(Bn * CTXP, C_))

    kd, vd = padded(k), padded(v)
    qd, od, dod = (G.bf(t.reshape(Bn * N, C_)) for t in (q, o, do))
    dq = torch.full((Bn * N, C_), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_cross_attn_bwd_q(_lib.ptr(qd), C_, _lib.ptr(kd), C_, _lib.ptr(vd), C_, _lib.ptr(od), C_, _lib.ptr(dod), C_,
                                            _lib.ptr(dq), C_, Bn, N, heads, d, None))
    G.sync()
    return dq.reshape(Bn, N, C_)


def test_cross_attn_bwd_q_never_reads_the_pad_rows(lib):
    B, heads, N, d = 2, 2, 128, 40
    c = attn_case(B, heads, N, d, keys=CTX)
    got = run_cross(lib, c, B, heads, N, d)
    assert torch.isfinite(got.float()).all()
    err = G.rel_err(got, c["dq"])
    print(f"cross_attn_bwd_q: {err:.3e}")
    G.within(err, 6e-3, what="cross_attn_bwd_q")


def test_attn_bwd_batch_rows_are_single_calls(lib):
    B, heads, N, d = 2, 2, 128, 40
    c = attn_case(B, heads, N, d)
    got = run_self(lib, c, B, heads, N, d, True)
    for b in range(B):
        one = run_self(lib, c, B, heads, N, d, True, rows=slice(b, b + 1))
        for g, o in zip(got, one):
            assert torch.equal(g[b:b + 1], o), b
    c = attn_case(B, heads, N, d, keys=CTX)
    got = run_cross(lib, c, B, heads, N, d)
    for b in range(B):
        assert torch.equal(got[b:b + 1], run_cross(lib, c, B, heads, N, d, rows=slice(b, b + 1))), b


def test_attn_bwd_rejects_bad_arguments(lib):
    buf = torch.zeros(1 << 18, dtype=dt(), device=G.dev())
    b = _lib.ptr(buf)

    def call(ldq=64, ldk=64, ldv=64, ldo=64, lddo=64, lddq=64, B=1, N=64, heads=2, d=32):
        return lib.hedit_k_attn_bwd(b, ldq, b, ldk, b, ldv, b, ldo, b, lddo, b, lddq, b, b, B, N, heads, d, b, None)

    assert call() == 0
    G.sync()
    for bad in (dict(N=96), dict(N=0), dict(d=48), dict(d=24, heads=2), dict(ldq=60), dict(ldk=32), dict(lddq=68), dict(ldv=56),
                dict(B=0)):
        assert call(**bad) == ERR_ARG, bad
    assert lib.hedit_k_cross_attn_bwd_q(b, 64, b, 64, b, 64, b, 64, b, 64, b, 64, 1, 100, 2, 32, None) == ERR_ARG
    assert lib.hedit_k_cross_attn_bwd_q(b, 64, b, 64, b, 64, b, 64, b, 64, b, 64, 1, 64, 2, 48, None) == ERR_ARG
    assert lib.hedit_k_cross_attn_bwd_q(b, 64, b, 32, b, 64, b, 64, b, 64, b, 64, 1, 64, 2, 32, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- LayerNorm / GEGLU backward
ROWS = 100            # ragged against any block size


@functools.lru_cache(maxsize=None)
def ln_case(Cw):
    x = st(hash_normal((ROWS, Cw), 31 + Cw) * 1.5 + 0.3)
    dy = st(hash_normal((ROWS, Cw), 32 + Cw))
    add = st(hash_normal((ROWS, Cw), 33 + Cw))
    gamma = 1.0 + 0.2 * hash_normal((Cw,), 34 + Cw)
    xd = x.double().requires_grad_(True)
    y = F.layer_norm(xd, (Cw,), gamma.double(), torch.zeros(Cw, dtype=torch.float64), 1e-5)
    (want,) = torch.autograd.grad(y, xd, dy.double())
    return x, dy, add, gamma, want


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("Cw", [64, 320, 1280])
def test_layernorm_bwd(lib, Cw, with_add):
    x, dy, add, gamma, want = ln_case(Cw)
    dx = torch.full((ROWS, Cw), float("nan"), dtype=dt(), device=G.dev())
    xd, dyd, addd = G.bf(x), G.bf(dy), G.bf(add)
    _lib.check(lib.hedit_k_layernorm_bwd(_lib.ptr(xd), _lib.ptr(dyd), _lib.ptr(addd) if with_add else None, _lib.ptr(dx),
                                         _lib.ptr(G.f32(gamma)), ROWS, Cw, 1e-5, None))
    G.sync()
    if with_add:
        want = want + add.double()
    assert torch.isfinite(dx.float()).all()
    G.within(G.rel_err(dx, want), 5e-3, what="layernorm_bwd")


def test_layernorm_bwd_rejects_bad_widths(lib):
    buf = torch.zeros(1 << 16, dtype=dt(), device=G.dev())
    g = torch.ones(4096, device=G.dev())
    for Cw in (60, 0, 2048):
        assert lib.hedit_k_layernorm_bwd(_lib.ptr(buf), _lib.ptr(buf), None, _lib.ptr(buf), _lib.ptr(g), 4, Cw, 1e-5, None) == ERR_ARG


@pytest.mark.parametrize("inner", [4 * 64, 4 * 320])
def test_geglu_bwd(lib, inner):
    x = st(hash_normal((ROWS, 2 * inner), 41 + inner) * 1.5)
    dy = st(hash_normal((ROWS, inner), 42 + inner))
    xd = x.double().requires_grad_(True)
    y = xd[:, :inner] * F.gelu(xd[:, inner:])
    (want,) = torch.autograd.grad(y, xd, dy.double())
    dx = torch.full((ROWS, 2 * inner), float("nan"), dtype=dt(), device=G.dev())
    xg, dyg = G.bf(x), G.bf(dy)
    _lib.check(lib.hedit_k_geglu_bwd(_lib.ptr(xg), _lib.ptr(dyg), _lib.ptr(dx), ROWS, inner, None))
    G.sync()
    assert torch.isfinite(dx.float()).all()
    G.within(G.rel_err(dx[:, :inner], want[:, :inner]), 5e-3, what="geglu_bwd value")
    G.within(G.rel_err(dx[:, inner:], want[:, inner:]), 5e-3, what="geglu_bwd gate")
    assert lib.hedit_k_geglu_bwd(_lib.ptr(xg), _lib.ptr(dyg), _lib.ptr(dx), ROWS, inner + 4, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- GroupNorm backward at concatenation widths
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("B,HW,Cw", [(2, 64, 960), (1, 256, 1920), (2, 64, 2560), (1, 1024, 2560)])
def test_groupnorm_bwd_at_concatenation_widths(lib, B, HW, Cw, with_add):
    """the widths of the SD UNet's skip concatenations: C / 8 no divisor of 256 (960, 1920) and above 256 (2560: the 512-thread
    blocks), against fp64 autograd through F.group_norm + SiLU on the stored operands with the statistics the forward kernel
    keeps; one slab per image and several"""
    Gn = 32
    x = st(hash_normal((B, HW, Cw), 61 + Cw + HW) * 1.5 + 0.2)
    dy = st(hash_normal((B, HW, Cw), 62 + Cw + HW))
    add = st(hash_normal((B, HW, Cw), 63 + Cw + HW))
    gamma, beta = 1.0 + 0.2 * hash_normal((Cw,), 64 + Cw), 0.1 * hash_normal((Cw,), 65 + Cw)
    xd = x.double().requires_grad_(True)
    y = F.silu(F.group_norm(xd.permute(0, 2, 1), Gn, gamma.double(), beta.double(), 1e-5))
    (want,) = torch.autograd.grad(y, xd, dy.double().permute(0, 2, 1))
    if with_add:
        want = want + add.double()
    xg, dyg, addg, gg, bg = G.bf(x), G.bf(dy), G.bf(add), G.f32(gamma), G.f32(beta)
    yg = torch.empty_like(xg)
    stats = torch.full((B, Gn, 2), float("nan"), device=G.dev())
    ws = torch.empty(max(lib.hedit_k_groupnorm_ws_bytes(B, HW, Cw), 16), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_k_groupnorm_stats(_lib.ptr(xg), _lib.ptr(yg), _lib.ptr(gg), _lib.ptr(bg), B, HW, Cw, Gn, 1e-5, 1, _lib.ptr(ws),
                                           _lib.ptr(stats), None))
    dx = torch.full((B, HW, Cw), float("nan"), dtype=dt(), device=G.dev())
    ws2 = torch.empty(max(lib.hedit_k_groupnorm_bwd_ws_bytes(B, HW, Cw), 16), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_k_groupnorm_bwd_any(_lib.ptr(xg), _lib.ptr(dyg), _lib.ptr(addg) if with_add else None, _lib.ptr(dx), _lib.ptr(gg),
                                             _lib.ptr(bg), _lib.ptr(stats), B, HW, Cw, Gn, 1, _lib.ptr(ws2), None))
    G.sync()
    assert torch.isfinite(dx.float()).all()
    G.within(G.rel_err(dx, want), 5e-3, what="groupnorm_bwd_any")
    assert lib.hedit_k_groupnorm_bwd_any(_lib.ptr(xg), _lib.ptr(dyg), None, _lib.ptr(dx), _lib.ptr(gg), _lib.ptr(bg), _lib.ptr(stats),
                                         B, HW, 4104 * 8, 8, 1, _lib.ptr(ws2), None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- stride-2, padding-1 conv input gradient
@functools.lru_cache(maxsize=None)
def s2p1_case(B, H, W, Cin, Cout):
    w = hash_normal((Cout, Cin, 3, 3), 51 + Cin + Cout) * (9 * Cin) ** -0.5
    dy = st(hash_normal((B, Cout, H // 2, W // 2), 53 + H + W))
    x = torch.zeros((B, Cin, H, W), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, st(w).double(), stride=2, padding=1)
    (want,) = torch.autograd.grad(y, x, dy.double())
    return w, dy, want


def s2p1_dgrad(lib, w, dy, H, W):
    B, Cout = dy.shape[:2]
    Cin = w.shape[1]
    wp = torch.empty(Cin * 9 * Cout, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_pack_conv3x3_s2_dgrad(_lib.ptr(G.f32(w)), _lib.ptr(wp), Cout, Cin, None))
    dyn = G.bf(dy.permute(0, 2, 3, 1))
    dx = torch.full((B, H, W, Cin), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_conv3x3_s2_dgrad_pad1(_lib.ptr(dyn), _lib.ptr(wp), _lib.ptr(dx), B, H, W, Cout, Cin, None))
    G.sync()
    return dx.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W,Cin,Cout", S2_SHAPES)
def test_s2_dgrad_pad1_matches_fp64_autograd(lib, B, H, W, Cin, Cout):
    w, dy, want = s2p1_case(B, H, W, Cin, Cout)
    got = s2p1_dgrad(lib, w, dy, H, W)
    assert torch.isfinite(got.float()).all()
    G.within(G.rel_err(got, want), 6e-3, what="s2 dgrad pad1")
    # row / column 0 are even pixels that only the centre tap reaches; the last row / column are odd pixels whose tap a = 0
    # falls outside dy
    for name, sl in (("last row", (slice(None), slice(None), H - 1)), ("last column", (slice(None), slice(None), slice(None), W - 1)),
                     ("row 0", (slice(None), slice(None), 0)), ("column 0", (slice(None), slice(None), slice(None), 0))):
        G.within(G.rel_err(got[sl], want[sl]), 6e-3, what="s2 dgrad pad1 " + name)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(3, 16, 16, 128, 128), (5, 64, 64, 128, 128)])
def test_s2_dgrad_pad1_batch_rows_are_single_calls(lib, B, H, W, Cin, Cout):
    w, dy, _ = s2p1_case(B, H, W, Cin, Cout)
    got = s2p1_dgrad(lib, w, dy, H, W)
    for b in (0, B - 1):
        assert torch.equal(s2p1_dgrad(lib, w, dy[b:b + 1], H, W), got[b:b + 1]), b


def test_s2_dgrad_pad1_rejects_odd_sizes_and_ragged_channels(lib):
    buf = torch.zeros(1 << 16, dtype=dt(), device=G.dev())
    for args in ((1, 7, 8, 64, 64), (1, 8, 8, 64, 96), (1, 8, 8, 32, 64)):
        assert lib.hedit_k_conv3x3_s2_dgrad_pad1(_lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), *args, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- the executor
ERR_STATE = -3
TOL_TINY = 2.5e-2          # tests/test_gpu_unet.py: one eps evaluation, bf16 pipeline vs fp32 oracle


class Net:
    """a HIP UNet with gradient, its oracle twin, and the raw C calls on its handle"""

    def __init__(self, config, seed):
        from hedit.unet import UNet2DConditionModel, random_state_dict
        self.cfg = dict(config)
        self.hip = UNet2DConditionModel(self.cfg, device=G.dev(), grad=True)
        self.sd = random_state_dict(self.hip.param_shapes, seed)
        self.hip.load_state_dict(self.sd)
        self.lib, self.h = self.hip._lib, self.hip._h
        self.ws = None

    @functools.cached_property
    def om(self):
        from oracle import sd_unet as OU
        om = OU.UNet2DConditionModel(**self.cfg).eval()
        om.load_state_dict(self.sd)
        for p in om.parameters():
            p.requires_grad_(False)
        return om

    def inputs(self, B, S, seed):
        x = hash_normal((B, 4, S, S), seed)
        ctx = hash_normal((B, 77, self.cfg["cross_attention_dim"]), seed + 1)
        u = hash_normal((B, 4, S, S), seed + 2)
        return x, ctx, u

    def workspace(self, B, S):
        need = self.lib.hedit_unet_grad_workspace_bytes(self.h, B, S, S)
        assert need > 0
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=G.dev())
        return self.ws

    def keep(self, x, t, ctx):
        B, S = x.shape[0], x.shape[2]
        ws = self.workspace(B, S)
        eps = torch.empty_like(x)
        _lib.check(self.lib.hedit_unet_forward_keep(self.h, _lib.ptr(x), float(t), _lib.ptr(ctx), B, S, S, _lib.ptr(eps), _lib.ptr(ws),
                                                    ws.numel(), None))
        return eps

    def backward(self, u):
        dx = torch.empty_like(u)
        _lib.check(self.lib.hedit_unet_backward(self.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(self.ws), None))
        G.sync()
        return dx

    def vjp(self, x, t, ctx, u):
        B, S = x.shape[0], x.shape[2]
        ws = self.workspace(B, S)
        dx, eps = torch.empty_like(x), torch.empty_like(x)
        _lib.check(self.lib.hedit_unet_vjp(self.h, _lib.ptr(x), float(t), _lib.ptr(ctx), _lib.ptr(u), B, S, S, _lib.ptr(dx), _lib.ptr(eps),
                                           _lib.ptr(ws), ws.numel(), None))
        G.sync()
        return dx, eps

    def oracle_vjp(self, x, t, ctx, u):
        xx = x.clone().requires_grad_(True)
        eps = self.om(xx, torch.tensor(t), encoder_hidden_states=ctx).sample
        (g,) = torch.autograd.grad((eps * u).sum(), xx)
        return g, eps.detach()


@pytest.fixture(scope="module")
def tiny():
    from hedit.unet import TINY_CONFIG
    return Net(TINY_CONFIG, 0)


# d = 40 and 80; 320 is the width the forward-only handle runs as chain kernels, whose unfused weights only the grad handle fills
SDW_CONFIG = dict(in_channels=4, out_channels=4, sample_size=32, block_out_channels=(320, 640, 640),
                  down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                  up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                  layers_per_block=2, cross_attention_dim=64, attention_head_dim=8, norm_num_groups=32)


def check_vjp(net, B, S, t, seed):
    x, ctx, u = net.inputs(B, S, seed)
    want, eps_want = net.oracle_vjp(x, t, ctx, u)
    got, eps = net.vjp(G.f32(x), t, G.f32(ctx), G.f32(u))
    assert got.shape == x.shape and torch.isfinite(got).all()
    e_eps, e_vjp = G.rel_err(eps, eps_want), G.rel_err(got, want)
    print(f"unet vjp B={B} S={S} t={t}: eps {e_eps:.3e} vjp {e_vjp:.3e}")
    G.within(e_eps, TOL_TINY, what="taped eps")
    G.within(e_vjp, 4e-2, what=f"unet vjp B={B} S={S}")
    return got, eps


@pytest.mark.parametrize("B,S,t", [(2, 32, 501.0), (3, 32, 21.0)])
def test_vjp_matches_oracle_autograd(tiny, B, S, t):
    check_vjp(tiny, B, S, t, 20 + B)


def test_vjp_sd_width_configuration():
    net = Net(SDW_CONFIG, 3)
    got, eps = check_vjp(net, 2, 32, 301.0, 40)
    x, ctx, u = (G.f32(v) for v in net.inputs(2, 32, 40))
    g1, e1 = net.vjp(x[1:].contiguous(), 301.0, ctx[1:].contiguous(), u[1:].contiguous())
    assert torch.equal(g1, got[1:]) and torch.equal(e1, eps[1:])
    # the forward-only route (chain kernels at 320) stays inside the same limit of the taped one's oracle
    plain = net.hip(x, 301.0, encoder_hidden_states=ctx, cross_attention_kwargs={"use_controller": False}).sample
    G.within(G.rel_err(plain, eps), TOL_TINY, what="forward vs taped forward")


def test_tape_semantics(tiny):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(2, 32, 50))
    v = G.f32(hash_normal((2, 4, 32, 32), 59))
    eps = tiny.keep(x, 501.0, ctx)
    a = tiny.backward(u)
    one_call, eps1 = tiny.vjp(x, 501.0, ctx, u)
    assert torch.equal(a, one_call) and torch.equal(eps1, eps)           # keep + backward == vjp
    tiny.keep(x, 501.0, ctx)
    a1 = tiny.backward(u)
    a2 = tiny.backward(u)                                                # a second backward on the same tape
    b = tiny.backward(v)                                                 # another cotangent on the same tape
    assert torch.equal(a1, a) and torch.equal(a2, a) and not torch.equal(a, b)
    tiny.keep(x, 501.0, ctx)
    assert torch.equal(tiny.backward(v), b)                              # == a fresh keep + backward


def test_vjp_is_linear(tiny):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(1, 32, 60))
    v = G.f32(hash_normal((1, 4, 32, 32), 69))
    tiny.keep(x, 301.0, ctx)
    a, b, c = tiny.backward(u), tiny.backward(v), tiny.backward(2.0 * u + v)
    G.within(G.rel_err(c, 2.0 * a + b), 2e-2, what="unet vjp linearity")


def test_batch_of_three_equals_single_calls(tiny):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(3, 32, 70))
    got, eps = tiny.vjp(x, 701.0, ctx, u)
    for i in range(3):
        gi, ei = tiny.vjp(x[i:i + 1].contiguous(), 701.0, ctx[i:i + 1].contiguous(), u[i:i + 1].contiguous())
        assert torch.equal(gi, got[i:i + 1]) and torch.equal(ei, eps[i:i + 1]), i


def test_error_paths(tiny):
    from hedit.unet import TINY_CONFIG, UNet2DConditionModel
    lib = tiny.lib
    x, ctx, u = (G.f32(v) for v in tiny.inputs(1, 32, 95))
    dx, eps = torch.empty_like(x), torch.empty_like(x)
    ws = tiny.workspace(1, 32)
    lib.hedit_unet_release(tiny.h)
    assert lib.hedit_unet_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None) == ERR_STATE      # nothing kept
    assert b"hedit_unet_forward_keep" in lib.hedit_last_error()
    tiny.keep(x, 501.0, ctx)
    other = torch.empty(4096, dtype=torch.uint8, device=G.dev())
    assert lib.hedit_unet_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(other), None) == ERR_ARG     # foreign workspace
    tiny.backward(u)                                                                                        # the tape survived
    lib.hedit_unet_release(tiny.h)
    assert lib.hedit_unet_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None) == ERR_STATE
    # a set hook
    hook_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
    fn = hook_t(lambda *a: 0)
    _lib.check(lib.hedit_unet_set_attn_hook(tiny.h, C.cast(fn, C.c_void_p), None))
    try:
        assert lib.hedit_unet_forward_keep(tiny.h, _lib.ptr(x), 501.0, _lib.ptr(ctx), 1, 32, 32, _lib.ptr(eps), _lib.ptr(ws), ws.numel(),
                                           None) == ERR_STATE
        assert b"hook" in lib.hedit_last_error()
    finally:
        _lib.check(lib.hedit_unet_set_attn_hook(tiny.h, None, None))
    # a forward-only handle
    plain = UNet2DConditionModel(TINY_CONFIG, device=G.dev())
    plain.load_state_dict(tiny.sd)
    assert lib.hedit_unet_grad_workspace_bytes(plain._h, 1, 32, 32) == 0
    assert lib.hedit_unet_forward_keep(plain._h, _lib.ptr(x), 501.0, _lib.ptr(ctx), 1, 32, 32, _lib.ptr(eps), _lib.ptr(ws), ws.numel(),
                                       None) == ERR_STATE
    assert b"hedit_unet_create_grad" in lib.hedit_last_error()
    assert lib.hedit_unet_vjp(plain._h, _lib.ptr(x), 501.0, _lib.ptr(ctx), _lib.ptr(u), 1, 32, 32, _lib.ptr(dx), _lib.ptr(eps), _lib.ptr(ws),
                              ws.numel(), None) == ERR_STATE
    assert plain.param_shapes == tiny.hip.param_shapes and not plain.grad
    # without grad=True nothing changes: no autograd node, the forward's bits
    out = plain(x.clone().requires_grad_(True), 501.0, encoder_hidden_states=ctx, cross_attention_kwargs={"use_controller": False}).sample
    assert not out.requires_grad
    with torch.no_grad():
        same = tiny.hip(x, 501.0, encoder_hidden_states=ctx, cross_attention_kwargs={"use_controller": False}).sample
    assert torch.equal(out, same)
    small = torch.empty(1 << 16, dtype=torch.uint8, device=G.dev())
    assert lib.hedit_unet_forward_keep(tiny.h, _lib.ptr(x), 501.0, _lib.ptr(ctx), 1, 32, 32, _lib.ptr(eps), _lib.ptr(small), small.numel(),
                                       None) == ERR_ARG
    assert b"workspace too small" in lib.hedit_last_error()
    assert lib.hedit_unet_forward_keep(tiny.h, _lib.ptr(x), 501.0, _lib.ptr(ctx), 1, 12, 16, _lib.ptr(eps), _lib.ptr(ws), ws.numel(),
                                       None) == ERR_ARG


def test_unet_is_an_autograd_node(tiny):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(2, 32, 80))
    kw = {"use_controller": False}
    want, eps_c = tiny.vjp(x, 401.0, ctx, u)
    xx = x.clone().requires_grad_(True)
    eps = tiny.hip(xx, torch.tensor(401), encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample
    assert eps.requires_grad and torch.equal(eps.detach(), eps_c)
    (g1,) = torch.autograd.grad((eps * u).sum(), xx, retain_graph=True)
    (g2,) = torch.autograd.grad((eps * (2 * u)).sum(), xx)
    G.sync()
    assert torch.equal(g1, want) and torch.equal(g2, tiny.vjp(x, 401.0, ctx, 2 * u)[0])
    # a graph whose forward was dropped by a later call says so
    e1 = tiny.hip(xx, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample
    tiny.hip(x, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw)
    with pytest.raises(RuntimeError, match="dropped"):
        torch.autograd.grad(e1.sum(), xx)
    with torch.no_grad():
        assert not tiny.hip(xx, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample.requires_grad
    # what the gradient pass cannot differentiate says which one is in the way
    with pytest.raises(NotImplementedError, match="encoder_hidden_states"):
        tiny.hip(xx, 401.0, encoder_hidden_states=ctx.clone().requires_grad_(True), cross_attention_kwargs=kw)
    from hedit.unet import AttnProcessor

    class Ctrl:
        def __call__(self, attn, is_cross, place, save_attn):
            return attn

    class Proc:
        controller = Ctrl()

    tiny.hip.set_attn_processor({k: Proc() for k in tiny.hip.attn_processors})
    try:
        with pytest.raises(NotImplementedError, match="registered controller"):
            tiny.hip(xx, 401.0, encoder_hidden_states=ctx)
        assert tiny.hip(xx, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample.requires_grad
    finally:
        tiny.hip.set_attn_processor({k: AttnProcessor() for k in tiny.hip.attn_processors})


# ---------------------------------------------------------------------------------------------- one NMG step, and the driver
def test_first_nmg_step_is_wired_to_the_gradient_pass():
    """One guidance update of nmg_p2p on the HIP pipeline, checked for wiring.  (A multi-step NMG run is not compared with the
    oracle loop: the loss is an L1 mean, so the cotangent is sign(residual) / numel, and with grad_scale = 5e3 and
    guidance_noise_map = 10 a last-bit difference flips signs that move the next step by O(1); see tests/test_host_nmg.py.)
    The step's x_rec recomputed in fp64 from the HIP model's own eps and gradient agrees to fp32 rounding, and the cotangent
    the step formed, pushed through the ORACLE's VJP, gives the HIP gradient within the whole-network limit.
    Measured: 1.5e-7 and 1.7e-2.  Under HEDIT_STORAGE=f16 (a hand run; this file is not in the half suite's list) the second
    figure is 3.0e-2 against the quarter limit 1e-2: the cotangent, sign(residual) c / numel ~ 7e-5 per element, sits at the
    edge of half's normal range, and the first layers' gradients are stored as subnormals."""
    from hedit.engine import HEditEngine, Schedule
    from hedit.inversion import p2p_baselines as PB
    from hedit.inversion.inversion_utils import encode_text, reverse_step
    from hedit.pipeline import HEditPipeline
    from hedit.scheduler import DDIMScheduler
    from hedit.unet import TINY_CONFIG, random_state_dict
    from oracle import sd_unet as OU
    hip = HEditPipeline.from_random(TINY_CONFIG, seed=0, device=G.dev(), text_layers=2, grad=True)
    hip.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    hip.scheduler.config.timestep_spacing = "leading"
    hip.scheduler.set_timesteps(10)
    w0 = G.f32(hash_normal((1, 4, 32, 32), 123) * 0.8)
    _, zs, wts = HEditEngine(hip).ddim_inversion(w0, ["a cat sitting on a bench"], 1.0)
    t = hip.scheduler.timesteps[0]
    x_rec, x_ori = wts[10].clone(), wts[9].clone()
    uncond = encode_text(hip, [""])
    plain = {"use_controller": False}
    eps_of = lambda x: hip.unet(x, t, encoder_hidden_states=uncond, cross_attention_kwargs=plain).sample      # noqa: E731
    got = PB._nmg_guide(hip, x_rec, x_ori, t, eps_of, 10.0, 5e3, False)
    # the same step by hand on the autograd facade
    x_in = x_rec.detach().requires_grad_(True)
    eps = eps_of(x_in)
    loss = F.l1_loss(reverse_step(hip, eps, t, x_in, eta=0.0), x_ori)
    (g_full,) = torch.autograd.grad(loss, x_in, retain_graph=True)
    (u,) = torch.autograd.grad(loss, eps, retain_graph=True)
    (g_net,) = torch.autograd.grad(eps, x_in, u)                        # a second backward on the same tape: J^T u alone
    G.sync()
    assert torch.isfinite(got).all() and g_full.abs().max() > 0
    S = Schedule(hip.scheduler)
    a_t, a_p = float(S.ab[int(t)]), float(S.ab_prev(int(t)))
    e64 = eps.detach().double()
    e_c = e64 - (1 - a_t) ** 0.5 * (-g_full.double()) * 5e3
    e_g = e64 + 10.0 * (e_c - e64)
    want = a_p ** 0.5 * (x_rec.double() - (1 - a_t) ** 0.5 * e_g) / a_t ** 0.5 + (1 - a_p) ** 0.5 * e_g
    err = G.rel_err(got, want)
    print(f"nmg step: x_rec vs fp64 recomputation {err:.3e}; guidance / plain update {G.rel_err(got, x_ori):.3e}")
    assert err < 1e-5
    om = OU.UNet2DConditionModel(**TINY_CONFIG).eval()
    om.load_state_dict(random_state_dict(hip.unet.param_shapes, 0))
    for p in om.parameters():
        p.requires_grad_(False)
    xx = x_rec.detach().cpu().requires_grad_(True)
    eps_o = om(xx, torch.tensor(int(t)), encoder_hidden_states=uncond.cpu()).sample
    (g_o,) = torch.autograd.grad((eps_o * u.cpu()).sum(), xx)
    e_vjp = G.rel_err(g_net, g_o)
    print(f"nmg step: HIP J^T u vs oracle J^T u {e_vjp:.3e}")
    G.within(e_vjp, 4e-2, what="nmg cotangent through the oracle")


def _nmg_driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hedit_main_nmg", os.path.join(ROOT, "h-edit_amd", "main_nmg.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


NMG_FLAGS = {"nmg": [], "nmg_p2p": ["--sa", "0.6"], "nmg_pnp": ["--pnp_f_t", "0.5", "--pnp_attn_t", "0.75"]}
NMG_TAIL = {"nmg": "_", "nmg_p2p": "_xa_0.4_sa0.6_", "nmg_pnp": "_f_t_0.5_attn_t_0.75_"}


@pytest.mark.parametrize("mode", list(NMG_FLAGS))
def test_nmg_driver_writes_edited_images(tmp_path, mode):
    """every mode from a PIE-Bench-style mapping file to finite 256 x 256 PNGs, and --batch 2 (lock-step, the L1 mean per
    image): byte-identical files"""
    import numpy as np
    from PIL import Image
    from helpers.datasets import pie_dataset as _dataset
    d = _dataset(tmp_path)
    common = ["--data_path", str(d), "--random_init", "--tiny", "--num_diffusion_steps", "4", "--edit_category_list", "0", "1",
              "--mode", mode] + NMG_FLAGS[mode]
    one = _nmg_driver().main(common + ["--output_path", str(tmp_path / "r1")])
    assert len(one) == 2                           # category 7 filtered out
    for p in one:
        sub = os.path.relpath(p, str(tmp_path / "r1")).split(os.sep)[0]
        assert sub.startswith(f"{mode}_total_steps_4_skip_0_implicit_False_eta_0.0_") and sub.endswith(NMG_TAIL[mode]), sub
        im = np.array(Image.open(p))
        assert im.shape == (256, 256, 3) and im.std() > 0
    two = _nmg_driver().main(common + ["--output_path", str(tmp_path / "r2"), "--batch", "2"])
    assert len(two) == 2
    for a, b in zip(sorted(one), sorted(two)):
        assert os.path.basename(a) == os.path.basename(b)
        assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b)))
