"""-m gpu: the pixel UNet's input-gradient pass (csrc/ddpm.hip: hedit_ddpm_forward_keep / _backward / _vjp on a handle
from hedit_ddpm_create_grad) and the two kernels it adds to the decoder's (csrc/s2dgrad.hip), against fp64 / fp32
torch.autograd on the CPU restatement that is pinned on the reference's own Model (tests/test_oracle_face.py).

Tolerances (relative L2, through G.within: half storage gets a quarter): 6e-3 for the stride-2 conv's input gradient, the
conv-dgrad limit of tests/test_gpu_grad_kernels.py; 4e-2 for the whole VJP, the project's limit for the decoder VJP built
from the same kernels (tests/test_gpu_vae.py); 2e-2 for linearity (ibid.).  For scale: bf16 autocast of the oracle moves
its own VJP by 1.4e-2.  What moves bits only is compared with torch.equal."""
import ctypes as C
import functools
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

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def dt():
    return _lib.storage_dtype()


# ---------------------------------------------------------------------------------------------- stride-2 conv input gradient
@functools.lru_cache(maxsize=None)
def s2_case(B, H, W, Cin, Cout):
    """operands rounded to the storage format, and the fp64 autograd gradient of the forward conv on them"""
    x_shape = (B, Cin, H, W)
    w = (hash_normal((Cout, Cin, 3, 3), 11 + Cin + Cout) * (9 * Cin) ** -0.5)
    dy = hash_normal((B, Cout, H // 2, W // 2), 13 + H + W).to(dt()).float()
    w_r = w.to(dt()).float()
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w_r.double(), stride=2)
    (want,) = torch.autograd.grad(y, x, dy.double())
    return w, dy, want                                    # want: (B, Cin, H, W) fp64


def s2_dgrad(lib, w, dy, H, W):
    """dy (B, Cout, H/2, W/2) fp32 -> dx (B, Cin, H, W) through the packed weight and the NHWC kernel"""
    B, Cout = dy.shape[:2]
    Cin = w.shape[1]
    wp = torch.empty(Cin * 9 * Cout, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_pack_conv3x3_s2_dgrad(_lib.ptr(G.f32(w)), _lib.ptr(wp), Cout, Cin, None))
    dyn = G.bf(dy.permute(0, 2, 3, 1))
    dx = torch.full((B, H, W, Cin), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_conv3x3_s2_dgrad(_lib.ptr(dyn), _lib.ptr(wp), _lib.ptr(dx), B, H, W, Cout, Cin, None))
    G.sync()
    return dx.permute(0, 3, 1, 2)


# the last: H != W catches a swap; 256 -> 256 takes the wider channel tile's weights; (5, 64 x 64) the 128-channel tile (Mq >= 4096)
S2_SHAPES = [(1, 8, 8, 64, 64), (2, 32, 32, 64, 64), (3, 16, 16, 128, 128), (1, 8, 16, 128, 64), (1, 16, 16, 256, 256),
             (5, 64, 64, 128, 128)]


@pytest.mark.parametrize("B,H,W,Cin,Cout", S2_SHAPES)
def test_s2_dgrad_matches_fp64_autograd(lib, B, H, W, Cin, Cout):
    w, dy, want = s2_case(B, H, W, Cin, Cout)
    got = s2_dgrad(lib, w, dy, H, W)
    assert torch.isfinite(got.float()).all()
    G.within(G.rel_err(got, want), 6e-3, what="s2 dgrad")
    # the borders separately (a whole-tensor norm hides them): the last row / column are odd pixels that only the centre tap
    # reaches, row / column 0 are even pixels whose second tap falls outside dy
    for name, sl in (("last row", (slice(None), slice(None), H - 1)), ("last column", (slice(None), slice(None), slice(None), W - 1)),
                     ("row 0", (slice(None), slice(None), 0)), ("column 0", (slice(None), slice(None), slice(None), 0))):
        G.within(G.rel_err(got[sl], want[sl]), 6e-3, what="s2 dgrad " + name)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(3, 16, 16, 128, 128), (5, 64, 64, 128, 128)])
def test_s2_dgrad_batch_rows_are_single_calls(lib, B, H, W, Cin, Cout):
    w, dy, _ = s2_case(B, H, W, Cin, Cout)
    got = s2_dgrad(lib, w, dy, H, W)
    for b in (0, B - 1):
        assert torch.equal(s2_dgrad(lib, w, dy[b:b + 1], H, W), got[b:b + 1]), b


def test_s2_dgrad_rejects_odd_sizes_and_ragged_channels(lib):
    buf = torch.zeros(1 << 16, dtype=dt(), device=G.dev())
    for args in ((1, 7, 8, 64, 64), (1, 8, 8, 64, 96), (1, 8, 8, 32, 64)):
        assert lib.hedit_k_conv3x3_s2_dgrad(_lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), *args, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- slice / accumulate
@pytest.mark.parametrize("ld,off,c", [(192, 0, 64), (192, 64, 128), (328, 200, 128), (72, 8, 64)])
def test_slice_add(lib, ld, off, c):
    M = 1000
    src = G.bf(hash_normal((M, ld), 5 + ld))
    dst0 = G.bf(hash_normal((M, c), 6 + off))
    dst = dst0.clone()
    _lib.check(lib.hedit_k_slice_add(_lib.ptr(src), ld, off, c, _lib.ptr(dst), M, 0, None))
    G.sync()
    assert torch.equal(dst, src[:, off:off + c])           # assign: exact
    dst = dst0.clone()
    _lib.check(lib.hedit_k_slice_add(_lib.ptr(src), ld, off, c, _lib.ptr(dst), M, 1, None))
    G.sync()
    assert torch.equal(dst, (dst0.float() + src[:, off:off + c].float()).to(dt()))      # fp32 add, one rounding
    assert lib.hedit_k_slice_add(_lib.ptr(src), ld, off + 4, c, _lib.ptr(dst), M, 0, None) == ERR_ARG
    assert lib.hedit_k_slice_add(_lib.ptr(src), ld, ld - c + 8, c, _lib.ptr(dst), M, 0, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------- the executor
class Net:
    """a HIP model with gradient, its oracle twin, and the raw C calls on its handle"""

    def __init__(self, config, seed):
        from hedit.diffusion import Model
        from oracle import ddpm_unet
        self.hip = Model(config, device=G.dev(), grad=True)
        sd = self.hip.init_random(seed)
        keys = ("in_channels", "out_ch", "ch", "ch_mult", "num_res_blocks", "attn_resolutions", "image_size")
        self.cfg = {k: self.hip.config[k] for k in keys}
        self.sd = sd
        self.lib, self.h = self.hip._lib, self.hip._h
        self.ws = None

    @functools.cached_property
    def om(self):
        from oracle import ddpm_unet
        om = ddpm_unet.Model(**self.cfg).eval()
        om.load_state_dict(self.sd)
        for p in om.parameters():
            p.requires_grad_(False)
        return om

    def workspace(self, B):
        need = self.lib.hedit_ddpm_grad_workspace_bytes(self.h, B)
        assert need > 0
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=G.dev())
        return self.ws

    def keep(self, x, t):
        ws = self.workspace(x.shape[0])
        eps = torch.empty_like(x)
        _lib.check(self.lib.hedit_ddpm_forward_keep(self.h, _lib.ptr(x), float(t), x.shape[0], _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None))
        return eps

    def backward(self, u):
        dx = torch.empty_like(u)
        _lib.check(self.lib.hedit_ddpm_backward(self.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(self.ws), None))
        G.sync()
        return dx

    def vjp(self, x, t, u):
        ws = self.workspace(x.shape[0])
        dx, eps = torch.empty_like(x), torch.empty_like(x)
        _lib.check(self.lib.hedit_ddpm_vjp(self.h, _lib.ptr(x), float(t), _lib.ptr(u), x.shape[0], _lib.ptr(dx), _lib.ptr(eps), _lib.ptr(ws),
                                           ws.numel(), None))
        G.sync()
        return dx, eps

    def oracle_vjp(self, x, t, u):
        xx = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad((self.om(xx, torch.ones(x.shape[0]) * t) * u).sum(), xx)
        return g


@pytest.fixture(scope="module")
def tiny():
    from hedit.diffusion import TINY_DDPM_CONFIG
    return Net(TINY_DDPM_CONFIG, 0)


def xu(B, S, seed):
    return hash_normal((B, 3, S, S), seed) * 0.8, hash_normal((B, 3, S, S), seed + 1)


@pytest.mark.parametrize("B,t", [(1, 1.0), (1, 991.0), (2, 501.0), (3, 1.0), (3, 991.0)])
def test_vjp_matches_oracle_autograd(tiny, B, t):
    x, u = xu(B, 32, 20 + B)
    want = tiny.oracle_vjp(x, t, u)
    got, _ = tiny.vjp(G.f32(x), t, G.f32(u))
    assert got.shape == x.shape and torch.isfinite(got).all()
    G.within(G.rel_err(got, want), 4e-2, what=f"ddpm vjp B={B} t={t}")


def test_vjp_deeper_configuration():
    """the configuration of test_unet_two_more_levels_and_blocks with a fourth level: two downsamples' and upsamples' worth of
    skip bookkeeping, attention inside the down and the up path, two blocks per level"""
    cfg = dict(in_channels=3, out_ch=3, ch=64, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=(16, 8), image_size=64)
    net = Net(cfg, 3)
    x, u = xu(2, 64, 40)
    want = net.oracle_vjp(x, 301.0, u)
    got, eps = net.vjp(G.f32(x), 301.0, G.f32(u))
    G.within(G.rel_err(got, want), 4e-2, what="ddpm vjp, 4 levels x 2 blocks")
    assert torch.equal(net.vjp(G.f32(x[1:]), 301.0, G.f32(u[1:]))[0], got[1:])


def test_taped_forward_and_tape_semantics(tiny):
    x, u = (G.f32(v) for v in xu(2, 32, 50))
    v = G.f32(hash_normal((2, 3, 32, 32), 59))
    plain = tiny.hip(x.clone(), 501.0)                                   # no grad requested: hedit_ddpm_forward
    eps = tiny.keep(x, 501.0)
    G.sync()
    assert torch.equal(eps, plain)                                       # nothing fuses at ch = 64: the same bits
    a = tiny.backward(u)
    one_call, eps1 = tiny.vjp(x, 501.0, u)
    assert torch.equal(a, one_call) and torch.equal(eps1, eps)           # keep + backward == vjp
    tiny.keep(x, 501.0)
    a1 = tiny.backward(u)
    a2 = tiny.backward(u)                                                # a second backward on the same tape
    b = tiny.backward(v)                                                 # another cotangent on the same tape
    assert torch.equal(a1, a) and torch.equal(a2, a)
    tiny.keep(x, 501.0)
    assert torch.equal(tiny.backward(v), b)                              # == a fresh keep + backward
    assert not torch.equal(a, b)


def test_vjp_is_linear(tiny):
    x, u = (G.f32(v) for v in xu(1, 32, 60))
    v = G.f32(hash_normal((1, 3, 32, 32), 69))
    tiny.keep(x, 301.0)
    a, b, c = tiny.backward(u), tiny.backward(v), tiny.backward(2.0 * u + v)
    G.within(G.rel_err(c, 2.0 * a + b), 2e-2, what="ddpm vjp linearity")


def test_batch_of_three_equals_single_calls(tiny):
    x, u = (G.f32(v) for v in xu(3, 32, 70))
    got, eps = tiny.vjp(x, 701.0, u)
    for i in range(3):
        gi, ei = tiny.vjp(x[i:i + 1].contiguous(), 701.0, u[i:i + 1].contiguous())
        assert torch.equal(gi, got[i:i + 1]) and torch.equal(ei, eps[i:i + 1]), i


def test_model_is_an_autograd_node(tiny):
    x, u = (G.f32(v) for v in xu(2, 32, 80))
    want, eps_c = tiny.vjp(x, 401.0, u)
    xx = x.clone().requires_grad_(True)
    eps = tiny.hip(xx, torch.ones(2) * 401.0)
    assert eps.requires_grad and torch.equal(eps.detach(), eps_c)
    (g1,) = torch.autograd.grad((eps * u).sum(), xx, retain_graph=True)
    (g2,) = torch.autograd.grad((eps * (2 * u)).sum(), xx)              # ef.py:95 / :106: two gradients from one forward
    G.sync()
    assert torch.equal(g1, want) and torch.equal(g2, tiny.vjp(x, 401.0, 2 * u)[0])
    # a graph whose forward was dropped by a later call says so
    e1 = tiny.hip(xx, 401.0)
    tiny.hip(x, 401.0)
    with pytest.raises(RuntimeError, match="dropped"):
        torch.autograd.grad(e1.sum(), xx)
    with torch.no_grad():
        assert not tiny.hip(xx, 401.0).requires_grad


def test_model_without_grad_behaves_as_before(tiny):
    from hedit.diffusion import Model, TINY_DDPM_CONFIG
    plain = Model(TINY_DDPM_CONFIG, device=G.dev())
    plain.load_state_dict(tiny.sd)
    x = G.f32(xu(2, 32, 90)[0])
    out = plain(x.clone().requires_grad_(True), 501.0)
    assert not out.requires_grad and not plain.grad
    assert torch.equal(out, tiny.hip(x, 501.0))
    assert plain.param_shapes == tiny.hip.param_shapes


def test_error_paths(tiny):
    from hedit.diffusion import Model, TINY_DDPM_CONFIG
    lib = tiny.lib
    x, u = (G.f32(v) for v in xu(1, 32, 95))
    dx = torch.empty_like(x)
    ws = tiny.workspace(1)
    lib.hedit_ddpm_release(tiny.h)
    assert lib.hedit_ddpm_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None) == ERR_STATE      # nothing kept
    assert b"hedit_ddpm_forward_keep" in lib.hedit_last_error()
    tiny.keep(x, 501.0)
    other = torch.empty(4096, dtype=torch.uint8, device=G.dev())
    assert lib.hedit_ddpm_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(other), None) == ERR_ARG      # foreign workspace
    assert b"workspace" in lib.hedit_last_error()
    tiny.backward(u)                                                                                         # the tape survived
    lib.hedit_ddpm_release(tiny.h)
    assert lib.hedit_ddpm_backward(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(ws), None) == ERR_STATE
    plain = Model(TINY_DDPM_CONFIG, device=G.dev())
    plain.load_state_dict(tiny.sd)
    eps = torch.empty_like(x)
    assert lib.hedit_ddpm_grad_workspace_bytes(plain._h, 1) == 0
    assert lib.hedit_ddpm_forward_keep(plain._h, _lib.ptr(x), 501.0, 1, _lib.ptr(eps), _lib.ptr(ws), ws.numel(), None) == ERR_STATE
    assert b"hedit_ddpm_create_grad" in lib.hedit_last_error()
    assert lib.hedit_ddpm_vjp(plain._h, _lib.ptr(x), 501.0, _lib.ptr(u), 1, _lib.ptr(dx), _lib.ptr(eps), _lib.ptr(ws), ws.numel(),
                              None) == ERR_STATE
    small = torch.empty(1 << 16, dtype=torch.uint8, device=G.dev())
    assert lib.hedit_ddpm_forward_keep(tiny.h, _lib.ptr(x), 501.0, 1, _lib.ptr(eps), _lib.ptr(small), small.numel(), None) == ERR_ARG
    assert b"workspace too small" in lib.hedit_last_error()


def test_celeba_shape_is_batch_invariant_and_matches_oracle():
    """CelebA-HQ configuration (113.7 M parameters, hash weights as test_celeba_shape_matches_oracle_and_is_batch_invariant):
    a batch's d_x rows are the bits of the single calls, and image 0 matches autograd through the oracle (a few seconds of
    CPU time at this size, so the comparison runs at the full 256 x 256)."""
    net = Net(None, 1)
    x, u = xu(2, 256, 5)
    xg, ug = G.f32(x), G.f32(u)
    got, eps = net.vjp(xg, 501.0, ug)
    assert torch.isfinite(got).all() and torch.isfinite(eps).all()
    for i in range(2):
        gi, ei = net.vjp(xg[i:i + 1].contiguous(), 501.0, ug[i:i + 1].contiguous())
        assert torch.equal(gi, got[i:i + 1]) and torch.equal(ei, eps[i:i + 1]), i
    want = net.oracle_vjp(x[:1], 501.0, u[:1])
    G.within(G.rel_err(got[:1], want), 4e-2, what="ddpm vjp, CelebA-HQ shape")
