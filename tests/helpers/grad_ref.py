"""fp64 restatements of the operations behind the image decoder's input-gradient kernels (csrc/grad.hip), written from the
formulas -- not from the kernels -- and pinned on torch.autograd by tests/test_host_grad_ref.py; plus the inputs of
tests/test_gpu_grad_kernels.py, built here so that the host test can assert, on the reference alone, that they exercise what
they are meant to (a term that is a rounding error of the answer checks nothing).

Layouts are the kernels': images NHWC ([B][HW][C] or [B][H][W][C]), weights as in the checkpoint (OIHW, [O][I])."""
import math

import torch

EPS = 1e-6          # the decoder's GroupNorm eps (diffusers AutoencoderKL)


def silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def group_stats(x, G, eps=EPS):
    """(mean, rstd) [B][G] in fp64 of x [B][HW][C], biased variance as in torch's GroupNorm"""
    B, HW, C = x.shape
    xg = x.double().reshape(B, HW, G, C // G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, (var + eps) ** -0.5


def groupnorm_bwd(x, dy, gamma, beta, mean, rstd, G, silu, add=None, terms=False):
    """Input gradient of y = act(gamma xh + beta), xh = (x - mean_g) rstd_g, act = SiLU or the identity, for the upstream dy;
    (mean, rstd) [B][G] are GIVEN (the kernel is handed the forward's fp32 pair), all arithmetic in fp64:
        t = dy act'(z) gamma ;  dx = rstd (t - mean_g(t) - xh mean_g(t xh)) (+ add)
    terms=True: also the two mean terms rstd mean_g(t) and rstd xh mean_g(t xh), broadcast to x's shape."""
    B, HW, C = x.shape
    cpg = C // G
    mu = mean.double()[:, None, :, None]
    r = rstd.double()[:, None, :, None]
    xh = (x.double().reshape(B, HW, G, cpg) - mu) * r
    ga = gamma.double().reshape(G, cpg)
    dz = dy.double().reshape(B, HW, G, cpg)
    if silu:
        dz = dz * silu_grad(xh * ga + beta.double().reshape(G, cpg))
    t = dz * ga
    m1 = t.mean(dim=(1, 3), keepdim=True)
    m2 = (t * xh).mean(dim=(1, 3), keepdim=True)
    term1 = (r * m1).expand_as(xh)
    term2 = r * xh * m2
    dx = (r * t - term1 - term2).reshape(B, HW, C)
    if add is not None:
        dx = dx + add.double()
    if terms:
        return dx, term1.reshape(B, HW, C), term2.reshape(B, HW, C)
    return dx


def softmax_fwd(s, scale):
    return torch.softmax(s.double() * scale, dim=-1)


def softmax_bwd(p, dp, scale, terms=False):
    """ds for p = softmax(scale s): ds = scale p (dp - rowsum(dp p)).  terms=True: also the row-dot term scale p rowsum(dp p)."""
    p, dp = p.double(), dp.double()
    dot = (dp * p).sum(dim=-1, keepdim=True)
    ds = scale * p * (dp - dot)
    return (ds, scale * p * dot) if terms else ds


def sum2x2(du):
    """backward of the nearest 2x upsample: du [B][2H][2W][C] -> [B][H][W][C], each input pixel collects its four copies"""
    B, H2, W2, C = du.shape
    return du.double().reshape(B, H2 // 2, 2, W2 // 2, 2, C).sum(dim=(2, 4))


def conv3x3_dgrad(dy, w):
    """input gradient of y = conv3x3(x, w), stride 1, zero padding 1: dy [B][H][W][O] NHWC, w [O][I][3][3] -> dx [B][H][W][I].
    y[p + (1 - ky, 1 - kx)] reads x[p] through tap (ky, kx), so dx[p] = sum_taps dy[p + (1 - ky, 1 - kx)] . w[:, :, ky, kx]."""
    B, H, W, O = dy.shape
    dyp = torch.zeros(B, H + 2, W + 2, O, dtype=torch.float64)
    dyp[:, 1:H + 1, 1:W + 1] = dy.double()
    wd = w.double()
    dx = torch.zeros(B, H, W, w.shape[1], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            sy, sx = 1 + (1 - ky), 1 + (1 - kx)
            dx += dyp[:, sy:sy + H, sx:sx + W] @ wd[:, :, ky, kx]
    return dx


def linear_dgrad(dy, w):
    """input gradient of y = x w^T: dy [M][O], w [O][I] -> [M][I]"""
    return dy.double() @ w.double()


def attention_grads(q, k, v, dO):
    """(dQ, dK, dV) of O = softmax(q k^T / sqrt(C)) v by fp64 autograd, q / k / v / dO [T][C]"""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(q @ k.t() / math.sqrt(q.shape[1]), dim=-1) @ v
    return torch.autograd.grad(o, (q, k, v), dO.double())


# ------------------------------------------------------------------------------------------ inputs of the GPU tests
GN_GROUPS = 32
# (B, HW, C): R = 256 / (C / 8) pixel rows per block.  (1, 1000, 64): R = 32, three ragged slabs; (3, 37, 512): R = 4, HW
# below one slab stride, B > 1; (1, 66000, 128): HW / 1024 = 64 slabs (the cap above 32) of 1032 pixels, the last one clamped;
# (1, 4483, 512): the apply pass cuts HW into 70 slabs of 65 pixels, 4550 in all -- its last slab starts past the image, empty
GN_SHAPES = [(2, 64, 128), (1, 1000, 64), (3, 37, 512), (1, 4096, 256), (1, 66000, 128), (1, 4483, 512)]
GN_TERM_SHARE = 0.5


def gn_case(B, HW, C, dtype, seed=None, G=GN_GROUPS):
    """x = 2 N(0,1) + 0.5 and dy = N(0,1) + 0.6 + 0.8 xh, both rounded to the storage format `dtype`: the offset feeds
    mean_g(t), the xh part feeds mean_g(t xh), so each mean term of the backward formula is most of dx -- with a random dy both
    are O(1 / sqrt(n)) of it.  Returns a dict of CPU tensors: x, dy, add (storage format), gamma, beta (fp32), mean, rstd (fp32
    [B][G], from the stored x in fp64)."""
    g = torch.Generator().manual_seed(B * 1000003 + HW * 101 + C if seed is None else seed)
    x = (torch.randn(B, HW, C, generator=g, dtype=torch.float64) * 2 + 0.5).to(dtype)
    mean, rstd = group_stats(x, G)
    cpg = C // G
    xh = ((x.double().reshape(B, HW, G, cpg) - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, HW, C)
    dy = (torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 0.6 + 0.8 * xh).to(dtype)
    add = torch.randn(B, HW, C, generator=g, dtype=torch.float64).to(dtype)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    return dict(x=x, dy=dy, add=add, gamma=gamma, beta=beta, mean=mean.float(), rstd=rstd.float(), G=G)


def gn_term_shares(case, silu):
    """(|| rstd mean_g(t) ||, || rstd xh mean_g(t xh) ||) / || dx ||, dx without the addend"""
    dx, t1, t2 = groupnorm_bwd(case["x"], case["dy"], case["gamma"], case["beta"], case["mean"], case["rstd"], case["G"], silu,
                               terms=True)
    n = dx.norm()
    return (t1.norm() / n).item(), (t2.norm() / n).item()


SM_N = [64, 256, 320, 1088]          # below, at and above one 256-element wave stride; 1088 = 4 strides + a quarter
SM_ROWS = [6, 64, 1088]              # 6: not a multiple of the 4 rows of a block
SM_SCALE = 1.0 / math.sqrt(2.0)      # not a power of two: scale, scale^2 and 1 are told apart
SM_DOT_SHARE = 0.5


def softmax_case(rows, N, seed=None):
    """scores s = 4 N(0,1) (peaked rows) and dp = N(0,1) + 3 (fp32): the offset is a row constant, which the row dot must cancel
    exactly -- what attention_bwd relies on when it drops the key and value biases"""
    g = torch.Generator().manual_seed(rows * 7919 + N if seed is None else seed)
    s = (4 * torch.randn(rows, N, generator=g)).float()
    dp = (torch.randn(rows, N, generator=g) + 3).float()
    return s, dp


def softmax_dot_share(p, dp, scale=SM_SCALE):
    ds, dot_term = softmax_bwd(p, dp, scale, terms=True)
    return (dot_term.norm() / ds.norm()).item()
