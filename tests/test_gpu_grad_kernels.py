"""-m gpu: the kernels of the image decoder's input-gradient pass (csrc/grad.hip) and the forward kernels that feed them
statistics and probabilities, one by one through the C ABI, against the fp64 restatements of tests/helpers/grad_ref.py (pinned on
torch.autograd by tests/test_host_grad_ref.py) evaluated on the same inputs after their rounding to the storage format.

Tolerances (relative L2, through G.within: half storage gets a quarter): 5e-3 for one 16-bit rounding of the output after fp32
arithmetic, 6e-3 where an MFMA GEMM is in the chain -- the conventions of tests/test_gpu_kernels.py.  What moves bits only
(transposes, weight re-packs, the zeros of the block-diagonal softmax, sums of exactly representable values, batch
independence) is compared with torch.equal.

The whole-network checks of tests/test_gpu_vae.py cannot see a slip in a mean term of the GroupNorm backward: with a random
upstream gradient both mean terms are O(1 / sqrt(n)) of the answer.  Here the inputs make each of them most of it
(grad_ref.gn_case / softmax_case; the host test asserts that on the reference alone)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import gpu as G  # noqa: E402
from helpers import grad_ref as R  # noqa: E402
from hedit import _lib  # noqa: E402

ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.lib()


def dt():
    return _lib.storage_dtype()


def bytes_buf(n):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=G.dev())


def run_gemm(lib, A, W, M, N, K, lda, ldc, mode=0, conv=(0, 0, 0, 0, 0)):
    out = torch.zeros(M, ldc, dtype=dt(), device=G.dev())
    ws = bytes_buf(lib.hedit_k_gemm_ws_bytes(M, N, K, 0))
    _lib.check(lib.hedit_k_gemm(_lib.ptr(A), _lib.ptr(W), None, None, _lib.ptr(out), M, N, K, lda, ldc, 0, mode, *conv, 0,
                                _lib.ptr(ws), None))
    G.sync()
    return out


# ---------------------------------------------------------------------------------------------- GroupNorm(+SiLU) backward
@functools.lru_cache(maxsize=None)
def gn_case(B, HW, C):
    """the inputs of a shape, on the host (for the reference) and on the device, built once"""
    c = R.gn_case(B, HW, C, dt())
    d = {k: (G.f32(v) if k in ("gamma", "beta") else G.bf(v)) for k, v in c.items() if k in ("x", "dy", "add", "gamma", "beta")}
    d["stats"] = G.f32(torch.stack((c["mean"], c["rstd"]), dim=-1))              # [B][G][2]
    return c, d


@functools.lru_cache(maxsize=None)
def gn_reference(B, HW, C, silu):
    c, _ = gn_case(B, HW, C)
    return R.groupnorm_bwd(c["x"], c["dy"], c["gamma"], c["beta"], c["mean"], c["rstd"], c["G"], silu)


def gn_bwd(lib, x, dy, add, gamma, beta, stats, B, HW, C, G_, silu):
    dx = torch.empty_like(x)
    ws = bytes_buf(lib.hedit_k_groupnorm_bwd_ws_bytes(B, HW, C))
    _lib.check(lib.hedit_k_groupnorm_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(add), _lib.ptr(dx), _lib.ptr(gamma), _lib.ptr(beta),
                                         _lib.ptr(stats), B, HW, C, G_, silu, _lib.ptr(ws), None))
    G.sync()
    return dx


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,C", R.GN_SHAPES)
def test_groupnorm_bwd(lib, B, HW, C, silu, with_add):
    """dx of groupnorm_bwd_launch == the fp64 formula on the stored x, dy (and addend) with the fp32 (mean, rstd) the kernel
    is handed.  The shapes: one slab; ragged slabs (HW = 1000 is no multiple of nslab * R); HW below one slab stride with
    B > 1; the decoder's own 64 x 64 x 256; gb_nslab's cap above 32 with a clamped last slab (and the apply kernel's own,
    larger slab count na); an apply slab that starts past the image and must do nothing."""
    c, d = gn_case(B, HW, C)
    got = gn_bwd(lib, d["x"], d["dy"], d["add"] if with_add else None, d["gamma"], d["beta"], d["stats"], B, HW, C, c["G"], silu)
    want = gn_reference(B, HW, C, silu)
    if with_add:
        want = want + c["add"].double()
    assert torch.isfinite(got.float()).all()
    G.within(G.rel_err(got, want), 5e-3, what="groupnorm_bwd")


@pytest.mark.parametrize("B,HW,C,silu", [(2, 64, 128, 1), (1, 1000, 64, 0), (1, 4096, 256, 1)])
def test_groupnorm_forward_keeps_the_stats_its_backward_needs(lib, B, HW, C, silu):
    """hedit_k_groupnorm_stats (the one-launch kernel of small images and the three-launch path) writes the same y as
    hedit_k_groupnorm, bit for bit, and (mean, rstd) within fp32 rounding of the fp64 statistics of the stored x; the backward
    on THOSE stats equals fp64 autograd through F.group_norm (+ SiLU).

    The statistics' bounds: any fixed-order fp32 sum of n terms is at least as accurate as the sequential one, whose error
    in the mean is a random walk of standard deviation ~ u |m| sqrt(n / 3) (u = 2^-24); 4 u sqrt(n) rms(x) is seven of those,
    plus one rounding of the result.  var = q / n - m^2 takes the same bound for the mean of squares, 2 |m| times the mean's, and
    a rounding of q / n; rstd = (var + eps)^-1/2 halves the relative error and adds the reciprocal square root's (2^-21)."""
    c, d = gn_case(B, HW, C)
    Gn = c["G"]
    y, y2 = torch.empty_like(d["x"]), torch.empty_like(d["x"])
    stats = torch.full((B, Gn, 2), float("nan"), device=G.dev())
    ws = bytes_buf(lib.hedit_k_groupnorm_ws_bytes(B, HW, C))
    _lib.check(lib.hedit_k_groupnorm_stats(_lib.ptr(d["x"]), _lib.ptr(y), _lib.ptr(d["gamma"]), _lib.ptr(d["beta"]), B, HW, C, Gn,
                                           R.EPS, silu, _lib.ptr(ws), _lib.ptr(stats), None))
    _lib.check(lib.hedit_k_groupnorm(_lib.ptr(d["x"]), _lib.ptr(y2), _lib.ptr(d["gamma"]), _lib.ptr(d["beta"]), B, HW, C, Gn,
                                     R.EPS, silu, _lib.ptr(ws), None))
    G.sync()
    assert torch.equal(y, y2)
    # statistics
    xg = c["x"].double().reshape(B, HW, Gn, C // Gn)
    n = HW * (C // Gn)
    m, r = R.group_stats(c["x"], Gn)
    u = 2.0 ** -24
    rms = (xg ** 2).mean(dim=(1, 3)).sqrt()
    rms2 = (xg ** 4).mean(dim=(1, 3)).sqrt()
    tol_m = 4 * u * math.sqrt(n) * rms + 2 * u * m.abs()
    tol_var = 4 * u * math.sqrt(n) * rms2 + 2 * u * rms ** 2 + 2 * m.abs() * tol_m
    tol_r = r * (0.5 * tol_var * r ** 2 + 2.0 ** -21)
    st = stats.double().cpu()
    em, er = (st[..., 0] - m).abs(), (st[..., 1] - r).abs()
    print(f"stats {B}x{HW}x{C}: mean err / bound {float((em / tol_m).max()):.3f}, rstd err / bound {float((er / tol_r).max()):.3f}")
    assert (em <= tol_m).all() and (er <= tol_r).all()
    # forward and backward together against autograd
    dx = gn_bwd(lib, d["x"], d["dy"], None, d["gamma"], d["beta"], stats, B, HW, C, Gn, silu)
    xa = c["x"].double().requires_grad_(True)
    ya = F.group_norm(xa.permute(0, 2, 1), Gn, c["gamma"].double(), c["beta"].double(), eps=R.EPS)
    if silu:
        ya = F.silu(ya)
    (want,) = torch.autograd.grad(ya, xa, c["dy"].double().permute(0, 2, 1))
    G.within(G.rel_err(y, ya.detach().permute(0, 2, 1)), 5e-3, what="groupnorm forward")
    G.within(G.rel_err(dx, want), 5e-3, what="groupnorm forward + backward vs autograd")


@pytest.mark.parametrize("HW,C", [(37, 512), (1000, 64)])
def test_groupnorm_bwd_is_batch_independent_and_repeatable(lib, HW, C):
    """gb_nslab is a function of (HW, C) only: the gradient of an image has the same bits alone and in a batch, and twice"""
    B = 3
    c, d = gn_case(B, HW, C)
    args = (d["gamma"], d["beta"])
    full = gn_bwd(lib, d["x"], d["dy"], d["add"], *args, d["stats"], B, HW, C, c["G"], 1)
    again = gn_bwd(lib, d["x"], d["dy"], d["add"], *args, d["stats"], B, HW, C, c["G"], 1)
    assert torch.equal(full, again)
    for b in range(B):
        one = gn_bwd(lib, d["x"][b:b + 1].contiguous(), d["dy"][b:b + 1].contiguous(), d["add"][b:b + 1].contiguous(), *args,
                     d["stats"][b:b + 1].contiguous(), 1, HW, C, c["G"], 1)
        assert torch.equal(full[b:b + 1], one), b


# ---------------------------------------------------------------------------------------------- softmax, forward and backward
@functools.lru_cache(maxsize=None)
def sm_case(rows, N):
    s, dp = R.softmax_case(rows, N)
    return s, dp, R.softmax_fwd(s, R.SM_SCALE)


def softmax_rows(lib, s, rows, N, scale):
    p = torch.full((rows, N), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_softmax_rows(_lib.ptr(s), _lib.ptr(p), rows, N, scale, None))
    G.sync()
    return p


@pytest.mark.parametrize("N", R.SM_N)
@pytest.mark.parametrize("rows", R.SM_ROWS)
def test_softmax_rows(lib, rows, N):
    """p == fp64 softmax(scale s) after one storage rounding, and the rows still sum to one as well as the rounding allows: the
    deviation of the fp64 row sum of the stored p from 1 at most twice that of the fp64 softmax rounded the same way."""
    s, _, want = sm_case(rows, N)
    p = softmax_rows(lib, G.f32(s), rows, N, R.SM_SCALE)
    G.within(G.rel_err(p, want), 5e-3, what="softmax_rows")
    dev = (p.double().cpu().sum(dim=-1) - 1).abs().max().item()
    dev_ref = (want.to(dt()).double().sum(dim=-1) - 1).abs().max().item()
    print(f"softmax rows {rows} x {N}: max |row sum - 1| {dev:.3e} (fp64 softmax rounded to storage: {dev_ref:.3e})")
    assert dev <= 2 * dev_ref, (dev, dev_ref)


@pytest.mark.parametrize("N", R.SM_N)
@pytest.mark.parametrize("rows", R.SM_ROWS)
def test_softmax_bwd(lib, rows, N):
    """ds == scale p (dp - rowsum(dp p)) in fp64 on the stored p.  dp carries a row constant of 3 that has to cancel: the row
    dot is most of the answer (host test), so a dot over too few elements, or none, fails here."""
    _, dp, pw = sm_case(rows, N)
    p = G.bf(pw)
    ds = torch.full((rows, N), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_softmax_bwd(_lib.ptr(p), _lib.ptr(G.f32(dp)), _lib.ptr(ds), rows, N, R.SM_SCALE, None))
    G.sync()
    assert torch.isfinite(ds.float()).all()
    G.within(G.rel_err(ds, R.softmax_bwd(p.cpu(), dp, R.SM_SCALE)), 5e-3, what="softmax_bwd")


@pytest.mark.parametrize("nimg", [2, 3])
def test_softmax_blockdiag(lib, nimg):
    """images stacked along both axes of one score matrix: exact zeros off the diagonal blocks (whatever the scores there), and
    each block bit-equal to softmax_rows on that image alone"""
    T = 64
    TG = nimg * T
    s = G.f32(4 * torch.randn(TG, TG, generator=torch.Generator().manual_seed(nimg)))
    p = torch.full((TG, TG), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_softmax_blockdiag(_lib.ptr(s), _lib.ptr(p), TG, T, TG, R.SM_SCALE, None))
    G.sync()
    off = torch.ones(TG, TG, dtype=torch.bool, device=G.dev())
    for b in range(nimg):
        blk = slice(b * T, (b + 1) * T)
        off[blk, blk] = False
        alone = softmax_rows(lib, s[blk, blk].contiguous(), T, T, R.SM_SCALE)
        assert torch.equal(p[blk, blk], alone), b
    assert (p.view(torch.int16)[off] == 0).all()         # +0.0, bit for bit


# ---------------------------------------------------------------------------------------------- transpose, 2x2 sums
@pytest.mark.parametrize("Rr,Cc", [(64, 64), (64, 192), (192, 64), (256, 128)])
def test_transpose(lib, Rr, Cc):
    src = G.bf(torch.randn(Rr, Cc, generator=torch.Generator().manual_seed(Rr * 3 + Cc)))
    dst = torch.full((Cc, Rr), float("nan"), dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_transpose(_lib.ptr(src), _lib.ptr(dst), Rr, Cc, None))
    G.sync()
    assert torch.equal(dst, src.t().contiguous())


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 64), (1, 8, 8, 128)])
def test_sum2x2(lib, B, H, W, C):
    """multiples of 2^-3 up to 2: the fp32 sum of four is exact, so the result is the fp64 sum rounded to storage, bit for bit;
    then random values at one output rounding"""
    g = torch.Generator().manual_seed(H * 10 + W)
    exact = torch.randint(-16, 17, (B, 2 * H, 2 * W, C), generator=g).double() / 8
    rand = torch.randn(B, 2 * H, 2 * W, C, generator=g)
    for du_h, bitwise in ((exact, True), (rand, False)):
        du = G.bf(du_h)
        dx = torch.full((B, H, W, C), float("nan"), dtype=dt(), device=G.dev())
        _lib.check(lib.hedit_k_sum2x2(_lib.ptr(du), _lib.ptr(dx), B, H, W, C, None))
        G.sync()
        want = R.sum2x2(du.cpu())
        if bitwise:
            assert torch.equal(du.cpu().double(), du_h)
            assert torch.equal(dx.cpu(), want.to(dt()))
        else:
            G.within(G.rel_err(dx, want), 5e-3, what="sum2x2")


# ---------------------------------------------------------------------------------------------- input-gradient GEMMs
def conv_dgrad(lib, dy, w, B, H, W, Cin, Cout):
    """dy [B][H][W][Cout] (storage) -> dx [B][H][W][Cin]: the forward 3x3 GEMM (mode 1) on the re-packed weight"""
    wq = torch.empty(Cin * 9 * Cout, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_pack_conv3x3_dgrad(_lib.ptr(G.f32(w)), _lib.ptr(wq), Cout, Cin, None))
    out = run_gemm(lib, dy, wq, B * H * W, Cin, 9 * Cout, Cout, Cin, mode=1, conv=(H, W, Cout, H, W))
    return out.reshape(B, H, W, Cin)


@pytest.mark.parametrize("Cin,Cout", [(64, 128), (128, 64)])
def test_conv3x3_dgrad(lib, Cin, Cout):
    """Cin != Cout both ways, H != W, B = 2: a transposed weight, unflipped taps or swapped H and W all fail"""
    B, H, W = 2, 8, 16
    g = torch.Generator().manual_seed(Cin)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    dy = G.bf(torch.randn(B, H, W, Cout, generator=g))
    got = conv_dgrad(lib, dy, w, B, H, W, Cin, Cout)
    want = R.conv3x3_dgrad(dy.cpu(), G.bf(w).cpu())
    xa = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    (auto,) = torch.autograd.grad(F.conv2d(xa, G.bf(w).cpu().double(), padding=1), xa, dy.cpu().double().permute(0, 3, 1, 2))
    assert G.rel_err(want, auto.permute(0, 2, 3, 1)) < 1e-10
    G.within(G.rel_err(got, want), 6e-3, what="conv3x3 dgrad")


def test_upsampling_conv3x3_dgrad(lib):
    """the gradient through conv(interpolate(x, 2, nearest)): the dgrad GEMM at the doubled resolution, then sum2x2"""
    B, H, W, Cin, Cout = 2, 4, 8, 64, 128
    g = torch.Generator().manual_seed(5)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    dy = G.bf(torch.randn(B, 2 * H, 2 * W, Cout, generator=g))
    du = conv_dgrad(lib, dy, w, B, 2 * H, 2 * W, Cin, Cout)
    dx = torch.empty(B, H, W, Cin, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_sum2x2(_lib.ptr(du), _lib.ptr(dx), B, H, W, Cin, None))
    G.sync()
    xa = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    ya = F.conv2d(F.interpolate(xa, scale_factor=2.0, mode="nearest"), G.bf(w).cpu().double(), padding=1)
    (want,) = torch.autograd.grad(ya, xa, dy.cpu().double().permute(0, 3, 1, 2))
    G.within(G.rel_err(dx, want.permute(0, 2, 3, 1)), 6e-3, what="upsampling conv3x3 dgrad")


def test_linear_dgrad(lib):
    M, I, O = 200, 128, 64
    g = torch.Generator().manual_seed(6)
    w = torch.randn(O, I, generator=g) / math.sqrt(I)
    dy = G.bf(torch.randn(M, O, generator=g))
    wt = torch.empty(I, O, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_pack_linear_t(_lib.ptr(G.f32(w)), _lib.ptr(wt), O, I, None))
    G.sync()
    assert torch.equal(wt, G.bf(w).t().contiguous())
    got = run_gemm(lib, dy, wt, M, I, O, O, I)
    xa = torch.zeros(M, I, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.linear(xa, G.bf(w).cpu().double()), xa, dy.cpu().double())
    assert G.rel_err(R.linear_dgrad(dy.cpu(), G.bf(w).cpu()), want) < 1e-10
    G.within(G.rel_err(got, want), 6e-3, what="linear dgrad")


@pytest.mark.parametrize("O,I,k", [(5, 3, 3), (8, 4, 1)])
def test_flip_oihw(lib, O, I, k):
    w = G.f32(torch.randn(O, I, k, k, generator=torch.Generator().manual_seed(k)))
    out = torch.full((I, O, k, k), float("nan"), device=G.dev())
    _lib.check(lib.hedit_k_flip_oihw(_lib.ptr(w), _lib.ptr(out), O, I, k, None))
    G.sync()
    assert torch.equal(out, w.flip(-1, -2).transpose(0, 1).contiguous())


# ---------------------------------------------------------------------------------------------- attention backward, composed
def test_attention_backward_composition(lib):
    """The entries above and hedit_k_gemm in the order attention_bwd (csrc/blocks.h) launches them for one image -- this test
    MIRRORS that function, it does not call it: P = softmax_rows(q k^T), dS = softmax_bwd(P, dO v^T), dV = P^T dO as
    gemm(transpose(P), transpose(dO)), dQ = dS k as gemm(dS, transpose(k)), dK = dS^T q as gemm(transpose(dS), transpose(q)) --
    against fp64 autograd of softmax(q k^T / sqrt(C)) v, dQ, dK and dV separately.  It pins which transpose feeds which GEMM
    (q and k have different statistics; T = C only in size).  The two fp32 score products (q k^T and dO v^T), which the
    executor takes from the GEMM's fp32 output -- not reachable through hedit_k_gemm --, are fp64 products of the stored
    operands rounded to fp32."""
    T = C = 64
    scale = 1 / math.sqrt(C)
    g = torch.Generator().manual_seed(8)
    q = G.bf(torch.randn(T, C, generator=g) * 1.2 + 0.3)
    k = G.bf(torch.randn(T, C, generator=g) * 0.7 - 0.2)
    v = G.bf(torch.randn(T, C, generator=g) + 0.1)
    dO = G.bf(torch.randn(T, C, generator=g) * 0.5 + 0.2)

    def f32_product(a, b):
        return G.f32(a.cpu().double() @ b.cpu().double().t())

    def transpose(src, rows, cols):
        dst = torch.empty(cols, rows, dtype=dt(), device=G.dev())
        _lib.check(lib.hedit_k_transpose(_lib.ptr(src), _lib.ptr(dst), rows, cols, None))
        return dst

    p = softmax_rows(lib, f32_product(q, k), T, T, scale)
    ds = torch.empty(T, T, dtype=dt(), device=G.dev())
    _lib.check(lib.hedit_k_softmax_bwd(_lib.ptr(p), _lib.ptr(f32_product(dO, v)), _lib.ptr(ds), T, T, scale, None))
    dv = run_gemm(lib, transpose(p, T, T), transpose(dO, T, C), T, C, T, T, C)
    dq = run_gemm(lib, ds, transpose(k, T, C), T, C, T, T, C)
    dk = run_gemm(lib, transpose(ds, T, T), transpose(q, T, C), T, C, T, T, C)
    want_q, want_k, want_v = R.attention_grads(q.cpu(), k.cpu(), v.cpu(), dO.cpu())
    G.within(G.rel_err(dv, want_v), 6e-3, what="attention dV")
    G.within(G.rel_err(dq, want_q), 6e-3, what="attention dQ")
    G.within(G.rel_err(dk, want_k), 6e-3, what="attention dK")


# ---------------------------------------------------------------------------------------------- outside the contract
def _gn_bwd_call(C, Gn):
    return lambda lib, b: lib.hedit_k_groupnorm_bwd(b, b, None, b, b, b, b, 1, 8, C, Gn, 1, b, None)


BAD_CALLS = {
    "groupnorm_bwd: C/8 = 24 is no divisor of 256": (_gn_bwd_call(192, 32), "groupnorm_bwd: C % 8, C % G, G <= 64, C/8 a divisor of 256"),
    "groupnorm_bwd: G = 128": (_gn_bwd_call(1024, 128), "groupnorm_bwd: C % 8, C % G, G <= 64, C/8 a divisor of 256"),
    "groupnorm_stats: G = 128": (lambda lib, b: lib.hedit_k_groupnorm_stats(b, b, b, b, 1, 8, 1024, 128, R.EPS, 1, b, b, None),
                                 "groupnorm: C % 8, C % G, G <= 64"),
    "softmax_rows: N = 66": (lambda lib, b: lib.hedit_k_softmax_rows(b, b, 4, 66, 1.0, None), "softmax_rows: N % 4"),
    "softmax_blockdiag: T = 6": (lambda lib, b: lib.hedit_k_softmax_blockdiag(b, b, 12, 6, 12, 1.0, None),
                                 "softmax_blockdiag: T % 4, ld % 4, rows % T"),
    "softmax_bwd: N = 66": (lambda lib, b: lib.hedit_k_softmax_bwd(b, b, b, 4, 66, 1.0, None), "softmax_bwd: N % 4"),
    "transpose: R = 32": (lambda lib, b: lib.hedit_k_transpose(b, b, 32, 64, None), "transpose: rows and columns must be multiples of 64"),
    "transpose: C = 96": (lambda lib, b: lib.hedit_k_transpose(b, b, 64, 96, None), "transpose: rows and columns must be multiples of 64"),
    "sum2x2: C = 12": (lambda lib, b: lib.hedit_k_sum2x2(b, b, 1, 2, 2, 12, None), "sum2x2: C % 8"),
    "pack_conv3x3_dgrad: no output": (lambda lib, b: lib.hedit_k_pack_conv3x3_dgrad(b, None, 8, 8, None), "pack args"),
    "pack_linear_t: no output": (lambda lib, b: lib.hedit_k_pack_linear_t(b, None, 8, 8, None), "pack args"),
    "flip_oihw: no output": (lambda lib, b: lib.hedit_k_flip_oihw(b, None, 8, 8, 3, None), "flip args"),
}


@pytest.mark.parametrize("name", list(BAD_CALLS))
def test_entry_outside_its_contract_is_an_argument_error(lib, name):
    """every entry keeps its launcher's ARG_CHECKs: HEDIT_ERR_ARG with the launcher's message, and nothing is launched (the
    buffer every pointer names -- large enough for the call's nominal shape -- keeps its bytes)"""
    call, message = BAD_CALLS[name]
    buf = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=G.dev())
    rc = call(lib, _lib.ptr(buf))
    G.sync()
    assert rc == ERR_ARG
    assert message in lib.hedit_last_error().decode()
    assert (buf == 0x5A).all()
