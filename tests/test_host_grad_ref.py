"""CPU: the fp64 restatements of tests/helpers/grad_ref.py (the yardstick of tests/test_gpu_grad_kernels.py) equal
torch.autograd.grad of the corresponding torch.nn.functional op in fp64 to 1e-10 relative, and the inputs the GPU tests feed the
kernels exercise what they are meant to: each mean term of the GroupNorm backward and the row dot of the softmax backward is at
least half of the answer, in both storage formats -- so a GPU test cannot pass with a term that is wrong or missing."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import grad_ref as R

DTYPES = [torch.bfloat16, torch.float16]
TOL = 1e-10


def rel(got, want):
    return ((got - want).norm() / want.norm()).item()


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B,HW,C,G", [(2, 37, 64, 32), (1, 100, 24, 3), (3, 16, 128, 32)])
def test_groupnorm_bwd_equals_autograd(B, HW, C, G, silu, with_add):
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(B, HW, C, generator=g, dtype=torch.float64) * 2 + 0.5
    dy = torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 0.3
    gamma = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    add = torch.randn(B, HW, C, generator=g, dtype=torch.float64) if with_add else None
    xa = x.clone().requires_grad_(True)
    y = F.group_norm(xa.permute(0, 2, 1), G, gamma, beta, eps=R.EPS)
    if silu:
        y = F.silu(y)
    (want,) = torch.autograd.grad(y, xa, dy.permute(0, 2, 1))
    if with_add:
        want = want + add
    mean, rstd = R.group_stats(x, G)
    assert rel(R.groupnorm_bwd(x, dy, gamma, beta, mean, rstd, G, silu, add), want) < TOL
    # the two mean terms are what takes the group's mean and its xh component out of rstd t: dx has neither left
    dx, t1, t2 = R.groupnorm_bwd(x, dy, gamma, beta, mean, rstd, G, silu, terms=True)
    xh = ((x.reshape(B, HW, G, C // G) - mean[:, None, :, None]) * rstd[:, None, :, None])
    dg = dx.reshape(B, HW, G, C // G)
    assert dg.mean(dim=(1, 3)).abs().max() < 1e-12 and (dg * xh).mean(dim=(1, 3)).abs().max() < 1e-6   # (eps: <xh, xh> = 1 - eps rstd^2)
    assert t1.norm() > 0 and t2.norm() > 0


@pytest.mark.parametrize("rows,N", [(6, 64), (5, 320)])
def test_softmax_bwd_equals_autograd_and_cancels_a_row_constant(rows, N):
    s, dp = (t.double() for t in R.softmax_case(rows, N))
    sa = s.clone().requires_grad_(True)
    p = F.softmax(sa * R.SM_SCALE, dim=-1)
    (want,) = torch.autograd.grad(p, sa, dp)
    assert rel(R.softmax_fwd(s, R.SM_SCALE), p.detach()) < TOL
    assert rel(R.softmax_bwd(p.detach(), dp, R.SM_SCALE), want) < TOL
    # dp + c gives the same ds: rows of p sum to one
    assert rel(R.softmax_bwd(p.detach(), dp + 7.0, R.SM_SCALE), want) < TOL
    ds, dot_term = R.softmax_bwd(p.detach(), dp, R.SM_SCALE, terms=True)
    assert rel(ds + dot_term, R.SM_SCALE * p.detach() * dp) < TOL


def test_sum2x2_equals_autograd_of_nearest_upsample():
    g = torch.Generator().manual_seed(1)
    B, H, W, C = 2, 3, 5, 4
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    du = torch.randn(B, 2 * H, 2 * W, C, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.interpolate(x, scale_factor=2.0, mode="nearest"), x, du.permute(0, 3, 1, 2))
    assert rel(R.sum2x2(du), want.permute(0, 2, 3, 1)) < TOL


@pytest.mark.parametrize("I,O", [(3, 5), (6, 2)])
def test_conv_and_linear_dgrad_equal_autograd(I, O):
    g = torch.Generator().manual_seed(I * 10 + O)
    B, H, W = 2, 4, 7
    x = torch.randn(B, I, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(O, I, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, O, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.conv2d(x, w, padding=1), x, dy.permute(0, 3, 1, 2))
    assert rel(R.conv3x3_dgrad(dy, w), want.permute(0, 2, 3, 1)) < TOL
    # through the upsampling convolution: the dgrad at the doubled resolution, then the 2x2 sums
    dy2 = torch.randn(B, 2 * H, 2 * W, O, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1), x, dy2.permute(0, 3, 1, 2))
    assert rel(R.sum2x2(R.conv3x3_dgrad(dy2, w)), want.permute(0, 2, 3, 1)) < TOL
    xl = torch.randn(9, I, generator=g, dtype=torch.float64, requires_grad=True)
    wl = torch.randn(O, I, generator=g, dtype=torch.float64)
    dl = torch.randn(9, O, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.linear(xl, wl), xl, dl)
    assert rel(R.linear_dgrad(dl, wl), want) < TOL


def test_attention_grads_equal_the_chain_of_restatements():
    """dO -> (dQ, dK, dV) by autograd == the formulas attention_bwd states (blocks.h), built from the restatements above"""
    g = torch.Generator().manual_seed(3)
    T, C = 12, 8
    q, k, v, dO = (torch.randn(T, C, generator=g, dtype=torch.float64) for _ in range(4))
    scale = 1 / math.sqrt(C)
    p = R.softmax_fwd(q @ k.t(), scale)
    ds = R.softmax_bwd(p, dO @ v.t(), scale)
    dq, dk, dv = R.attention_grads(q, k, v, dO)
    assert rel(ds @ k, dq) < TOL and rel(ds.t() @ q, dk) < TOL and rel(p.t() @ dO, dv) < TOL


# ------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,C", R.GN_SHAPES)
def test_gn_inputs_make_each_mean_term_most_of_the_answer(B, HW, C, silu, dtype):
    s1, s2 = R.gn_term_shares(R.gn_case(B, HW, C, dtype), silu)
    assert s1 >= R.GN_TERM_SHARE and s2 >= R.GN_TERM_SHARE, (s1, s2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", R.SM_N)
@pytest.mark.parametrize("rows", R.SM_ROWS)
def test_softmax_inputs_are_peaked_and_the_row_dot_is_most_of_the_answer(rows, N, dtype):
    s, dp = R.softmax_case(rows, N)
    p = R.softmax_fwd(s, R.SM_SCALE).to(dtype)
    assert R.softmax_dot_share(p, dp) >= R.SM_DOT_SHARE
    assert p.double().max(dim=-1).values.median() > 8.0 / N          # peaked: far from the flat 1 / N
