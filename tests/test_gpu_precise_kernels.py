"""-m gpu: the kernels of the "precise" (split-bf16) path one by one through the C ABI (the `hedit_k_*` entries of the precise family in
include/hedit.h) against fp64 references on the same inputs: csrc/pnet.hip, csrc/encoder.hip, the attention / LayerNorm gradient
kernels of csrc/vit.hip and one layer as the executors run it (op_split + pgemm of csrc/pnet.h).

What is asserted (tests/helpers/precise_ref.py has the derivations, tests/test_host_precise_ref.py shows on the CPU that the product
bound rejects a product with a missing cross term):
* the split operand: layout, padding and dead rows exact zeros, both hi copies identical, hi + lo within 2^-16 |v| of the fp64 op;
* the packed weight bit for bit;
* the product within 3 * 2^-16 * |a| |w|^T + the fp32 accumulation term, and 2^-14 relative L2, against fp64 conv2d / autograd;
* fp32 kernels: torch.equal with an fp32 restatement where only single roundings happen, else (n + 2) 2^-24 sum |terms| (+ the fast
  exponential's (|x| + 4) 2^-23) with the chain lengths written at each test; gradients against fp64 autograd of the forward.
Every input sits between NaN margins, every output inside a sentinel band, and every launch runs twice with identical bits.
The operands are bfloat16 by contract in both storage builds, so nothing here depends on HEDIT_STORAGE."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import gemm_ref as GR  # noqa: E402
from helpers import gpu as G  # noqa: E402
from helpers import precise_ref as R  # noqa: E402
from hedit import _lib  # noqa: E402

U = R.U32
MG = R.Margins()
ptr = _lib.ptr


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gi(t):
    """device copy between NaN margins (None stays None)"""
    return None if t is None else R.nan_guarded(t, G.dev())


def gi2(t, ld):
    """[rows][cols] device copy at row stride ld, NaN padding columns and margins"""
    return None if t is None else GR.guarded(t.float().to(G.dev()), ld, 64)[0]


def run2(what, sizes, call, finite=True):
    """call(*fp32 windows of the given sizes) twice, each on fresh sentinel buffers: the bands stay, every element is written, the
    two launches agree bit for bit.  Returns the windows of the first launch."""
    res = []
    for _ in range(2):
        bufs = [R.out32(n, G.dev()) for n in sizes]
        call(*[w for w, _ in bufs])
        G.sync()
        for (w, b), n in zip(bufs, sizes):
            R.check_guard32(b, n, what, finite=finite)
        res.append([w.clone() for w, _ in bufs])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: a second launch gives other bits"
    return res[0]


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def spread(shape, g, lo=-3.0, hi=3.0):
    """normal values with magnitudes spread over 2^lo .. 2^hi"""
    return torch.randn(shape, generator=g) * torch.exp2(torch.rand(shape, generator=g) * (hi - lo) + lo)


# ------------------------------------------------------------------------------------------------------------------ split3
def split3_inputs(rows, C, op, with_q, pq_img, B, seed):
    g = gen(seed)
    x = spread((rows, C), g, -2, 2)
    shape = (B, C) if pq_img else (C,)
    p = torch.randn(shape, generator=g) if op in R.AFFINE_OPS + (R.P_PRELU, R.P_PRELU_GRAD) else None
    q = torch.randn(shape, generator=g) if (with_q or op in R.AFFINE_OPS) else None
    z = None
    if op in R.GRAD_OPS:
        z = torch.randn(rows, C, generator=g)            # its own signs
        t = z + (q.reshape(1, C) if q is not None else 0)
        z = torch.where(t.abs() < 2.0 ** -10, z + 0.5, z)      # the mask is a step function of t: keep t away from 0
    return x, z, p, q


def split3_case(lib, x, C, ldx, op, z, p, q, pq_img, geo, B, H, W, worder, what):
    Cs, Kp = R.split_cs(C), R.split_kp(C)
    cs, kp = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.hedit_k_split3_geometry(C, ctypes.byref(cs), ctypes.byref(kp)))
    assert (cs.value, kp.value) == (Cs, Kp)
    ref = R.split3_ref(x, C, op, z, p, q, pq_img, geo, B, H, W)
    rows_out = ref["v"].shape[0]
    xd, zd, pd, qd = gi2(x, ldx), gi2(z, ldx), gi(p), gi(q)

    def call(out):
        _lib.check(lib.hedit_k_split3(ptr(xd), ldx, ptr(zd), ptr(pd), ptr(qd), pq_img, op, ptr(out), Kp, Cs, C, geo, B, H, W, worder,
                                      rows_out, None))

    (o,) = run2(what, [rows_out * Kp // 2], call, finite=False)
    bits = o.view(torch.int16).view(rows_out, Kp).cpu()
    vals = bits.view(torch.bfloat16).double()
    assert torch.isfinite(vals).all(), f"{what}: non-finite operand (an input read past its extent?)"
    hi_c, hi2_c, lo_c, pad = R.split3_columns(C, worder)
    assert bool((bits[:, pad] == 0).all()), f"{what}: padding columns are not exact zeros"
    assert torch.equal(bits[:, hi_c], bits[:, hi2_c]), f"{what}: the two hi copies differ"
    assert bool((bits[~ref["live"]] == 0).all()), f"{what}: dead rows of the zero-stuffed geometry are not exact zeros"
    v, allow = ref["v"], ref["allow"]
    R.check_bound(vals[:, hi_c] + vals[:, lo_c], v, 2.0 ** -16 * (v.abs() + allow) + allow, f"split3 {what}", MG)
    # hi is the bfloat16 nearest the value: within half an ulp (2^-8 relative covers it) of the fp64 op
    R.check_bound(vals[:, hi_c], v, 2.0 ** -8 * (v.abs() + allow) + allow, f"split3_hi {what}")
    if op == R.P_COPY:
        xs = x.float()[ref["src"]]
        xs[~ref["live"]] = 0
        hi, lo = R.hi_lo(xs)
        assert torch.equal(bits[:, hi_c], hi.to(torch.bfloat16).view(torch.int16)), f"{what}: hi bits"
        assert torch.equal(bits[:, lo_c], lo.to(torch.bfloat16).view(torch.int16)), f"{what}: lo bits"
    return bits


def op_variants():
    for op in range(10):
        for with_q in ((True,) if op in R.AFFINE_OPS else ((False,) if op == R.P_COPY else (False, True))):
            yield op, with_q


SPLIT_C = [3, 8, 20, 24, 64, 72, 100, 200]


@pytest.mark.parametrize("pad", [0, 4, 1], ids=["ldx=C", "ldx=C+4", "ldx=C+1"])
@pytest.mark.parametrize("C", SPLIT_C)
def test_split3_ops(lib, C, pad):
    """all ten ops (q null and given where the op allows), both part orders, 37 rows (several blocks, a ragged last one); p / q per
    (image, channel) with three images under the affine ops.  ldx = C + 1 forces the one-column kernel at C % 8 == 0."""
    ldx = C + pad
    for op, with_q in op_variants():
        for worder in (0, 1):
            x, z, p, q = split3_inputs(37, C, op, with_q, 0, 1, 100 * C + op)
            split3_case(lib, x, C, ldx, op, z, p, q, 0, 0, 1, 37, 1, worder, f"{R.OP_NAMES[op]} C={C} ldx={ldx} q={with_q} worder={worder}")
    for op in R.AFFINE_OPS:
        x, z, p, q = split3_inputs(45, C, op, True, 1, 3, 7 * C + op)
        split3_case(lib, x, C, ldx, op, z, p, q, 1, 0, 3, 5, 3, 0, f"{R.OP_NAMES[op]} C={C} ldx={ldx} pq_img B=3")


@pytest.mark.parametrize("pad", [0, 1], ids=["ldx=C", "ldx=C+1"])
@pytest.mark.parametrize("C", [3, 24, 72])
def test_split3_geometries(lib, C, pad):
    """geo 1 (every second pixel of every second row, B = 2, 6 x 4) and geo 2 (zero-stuffed, B = 2, 3 x 5; also with the per-image
    affine the SE gradient feeds through it): rows against the index restatement, dead rows exact zeros"""
    ldx = C + pad
    for worder in (0, 1):
        x, z, p, q = split3_inputs(2 * 6 * 4, C, R.P_COPY, False, 0, 2, C + 1)
        split3_case(lib, x, C, ldx, R.P_COPY, None, None, None, 0, 1, 2, 6, 4, worder, f"geo1 copy C={C} ldx={ldx} worder={worder}")
        x, z, p, q = split3_inputs(2 * 3 * 5, C, R.P_COPY, False, 0, 2, C + 2)
        split3_case(lib, x, C, ldx, R.P_COPY, None, None, None, 0, 2, 2, 3, 5, worder, f"geo2 copy C={C} ldx={ldx} worder={worder}")
    x, z, p, q = split3_inputs(2 * 3 * 5, C, R.P_AFFINE, True, 1, 2, C + 3)
    split3_case(lib, x, C, ldx, R.P_AFFINE, None, p, q, 1, 2, 2, 3, 5, 0, f"geo2 affine pq_img C={C} ldx={ldx}")
    x, z, p, q = split3_inputs(2 * 6 * 4, C, R.P_PRELU_GRAD, True, 0, 2, C + 4)
    split3_case(lib, x, C, ldx, R.P_PRELU_GRAD, z, p, q, 0, 1, 2, 6, 4, 0, f"geo1 prelu_grad C={C} ldx={ldx}")


def test_split3_wide_and_narrow_kernels_agree(lib):
    """C = 24 at ldx 24 (eight columns per thread) and at ldx 25 (one): the same bits for every op on the same data"""
    C = 24
    for op, with_q in op_variants():
        x, z, p, q = split3_inputs(37, C, op, with_q, 0, 1, 900 + op)
        a = split3_case(lib, x, C, 24, op, z, p, q, 0, 0, 1, 37, 1, 0, f"wide {R.OP_NAMES[op]} q={with_q}")
        b = split3_case(lib, x, C, 25, op, z, p, q, 0, 0, 1, 37, 1, 0, f"narrow {R.OP_NAMES[op]} q={with_q}")
        assert torch.equal(a, b), f"{R.OP_NAMES[op]} q={with_q}: the two split3 kernels disagree"


# ------------------------------------------------------------------------------------------------------------------ packed weights
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("O,I,k,perm_hw,perm_c", [(5, 3, 3, 0, 0), (64, 24, 3, 0, 0), (10, 100, 1, 0, 0), (6, 48, 1, 4, 12)])
def test_pack_split3_w(lib, O, I, k, perm_hw, perm_c, dgrad, scaled):
    g = gen(O * 1000 + I)
    w = spread((O, I, k, k), g)
    scale = torch.randn(O, generator=g) if scaled else None
    NR, NC = (I, O) if dgrad else (O, I)
    rows = (NR + 3) // 4 * 4
    Cs, Kp = R.split_cs(NC), R.split_kp(NC)
    wd, sd = gi(w), gi(scale)

    def call(out):
        _lib.check(lib.hedit_k_pack_split3_w(ptr(wd), ptr(sd), ptr(out), O, I, k, dgrad, Cs, Kp, rows, perm_hw, perm_c, None))

    (o,) = run2("pack_split3_w", [rows * k * k * Kp // 2], call, finite=False)
    got = o.view(torch.int16).view(rows, k * k, Kp).cpu()
    want = R.pack_w_ref(w, scale, O, I, k, dgrad, rows, perm_hw, perm_c)
    assert bool((got[NR:] == 0).all()), "padded rows are not exact zeros"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} packed elements differ"


# ------------------------------------------------------------------------------------------------------------------ the product
def nhwc_rows(t):      # [B][C][H][W] -> [B H W][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_reference(x_rows, w, scale, B, H, W, mode, dgrad, pre=None):
    """(ref, mag) fp64 [M][channels out] of the layer on x_rows [B H W][Cin] (already through op and geo: `pre` maps the raw rows to the
    operand values in fp64).  Forward: conv2d.  dgrad: autograd of conv2d w.r.t. its input with x_rows as the output gradient.  mag is
    the same with absolute values (the layer is linear in both operands)."""
    O, I, k = w.shape[0], w.shape[1], w.shape[2]
    w64 = w.double() * (scale.double().reshape(O, 1, 1, 1) if scale is not None else 1)
    a = x_rows.double() if pre is None else pre
    stride, padding = (2 if mode == 2 else 1), (0 if mode == 0 else 1)

    def layer(inp, wt):
        return F.conv2d(inp, wt, stride=stride, padding=padding)

    out = []
    for aa, ww in ((a, w64), (a.abs(), w64.abs())):
        if not dgrad:
            out.append(nhwc_rows(layer(aa.reshape(B, H, W, I).permute(0, 3, 1, 2), ww)))
        else:
            Hi, Wi = (2 * H, 2 * W) if mode == 2 else (H, W)
            xin = torch.zeros(B, I, Hi, Wi, dtype=torch.float64, requires_grad=True)
            (gx,) = torch.autograd.grad(layer(xin, ww), xin, aa.reshape(B, H, W, O).permute(0, 3, 1, 2))
            out.append(nhwc_rows(gx))
    return out[0], out[1]


def precise_conv(lib, x, w, scale, dgrad, mode, B, Hin, Win, op=R.P_COPY, p=None, q=None, pq_img=0, z=None, geo=0, perm=(0, 0), what=""):
    """-> (out [M][rows] on the host, chunk_kt, splits)"""
    O, I, k = w.shape[0], w.shape[1], w.shape[2]
    rows = ((I if dgrad else O) + 3) // 4 * 4
    Hs, Ws = {0: (Hin, Win), 1: (Hin // 2, Win // 2), 2: (2 * Hin, 2 * Win)}[geo]
    M = B * Hs * Ws // (4 if mode == 2 else 1)
    need = lib.hedit_k_precise_conv_ws_bytes(O, I, k, dgrad, mode, geo, B, Hin, Win)
    assert need > 0, lib.hedit_last_error()
    xd, wd, sd, pd, qd, zd = gi(x), gi(w), gi(scale), gi(p), gi(q), gi(z)
    ck, sp = ctypes.c_int(-1), ctypes.c_int(-1)

    def call(out):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=G.dev())        # NaN in either format
        _lib.check(lib.hedit_k_precise_conv(ptr(xd), op, ptr(pd), ptr(qd), pq_img, ptr(zd), geo, ptr(wd), ptr(sd), O, I, k, perm[0], perm[1],
                                            dgrad, mode, B, Hin, Win, ptr(out), ctypes.byref(ck), ctypes.byref(sp), ptr(ws), need, None))

    (o,) = run2(f"precise_conv {what}", [M * rows], call)
    return o.view(M, rows).cpu(), ck.value, sp.value


def product_case(lib, what, O, I, k, mode, B, H, W, seed, scaled=False):
    """forward and input gradient of one layer against fp64; the padded output columns are exact zeros"""
    g = gen(seed)
    w = spread((O, I, k, k), g, -2, 2) / math.sqrt(I * k * k)
    scale = (torch.rand(O, generator=g) + 0.5) if scaled else None
    x = spread((B * H * W, I), g)
    got, ck, sp = precise_conv(lib, x, w, scale, 0, mode, B, H, W, what=what)
    ref, mag = conv_reference(x, w, scale, B, H, W, mode, False)
    assert bits_equal(got[:, O:], torch.zeros_like(got[:, O:])), f"{what}: padded output columns are not exact zeros"
    R.check_product(got[:, :O], ref, mag, k * k * R.split_kp(I), f"product_fwd {what}", MG)
    Ho, Wo = (H // 2, W // 2) if mode == 2 else (H, W)
    dy = spread((B * Ho * Wo, O), g)
    gref, gmag = conv_reference(dy, w, scale, B, Ho, Wo, mode, True)
    if mode == 2:        # the composition the executors use: zero-stuff to the input size, then the stride-1 input gradient
        ggot, _, _ = precise_conv(lib, dy, w, scale, 1, 1, B, Ho, Wo, geo=2, what=what + " dgrad")
    else:
        ggot, _, _ = precise_conv(lib, dy, w, scale, 1, mode, B, Ho, Wo, what=what + " dgrad")
    assert bits_equal(ggot[:, I:], torch.zeros_like(ggot[:, I:])), f"{what}: padded gradient columns are not exact zeros"
    R.check_product(ggot[:, :I], gref, gmag, k * k * R.split_kp(O), f"product_dgrad {what}", MG)
    return ck, sp


def test_product_linear(lib):
    """M = 37 rows, 100 -> 10 channels: one plain chain (K = 384), rows padded to 12"""
    product_case(lib, "linear 37x100->10", 10, 100, 1, 0, 1, 37, 1, 1)
    product_case(lib, "linear 37x100->10 scaled", 10, 100, 1, 0, 1, 37, 1, 2, scaled=True)


def test_product_conv3x3(lib):
    """3 x 3 stride 1, B = 2, 6 x 4, 24 -> 5 channels: rows padded to 8, columns 5..7 exact zeros"""
    product_case(lib, "conv3x3 s1 2x6x4 24->5", 5, 24, 3, 1, 2, 6, 4, 3)
    product_case(lib, "conv3x3 s1 2x6x4 24->5 scaled", 5, 24, 3, 1, 2, 6, 4, 4, scaled=True)


def test_product_conv3x3_stride2(lib):
    """3 x 3 stride 2, 8 x 8 -> 4 x 4 (mode 2); its gradient is geo 2 zero-stuffing + the mode-1 input gradient"""
    product_case(lib, "conv3x3 s2 2x8x8 8->6", 6, 8, 3, 2, 2, 8, 8, 5)
    product_case(lib, "conv3x3 s2 1x8x8 72->20", 20, 72, 3, 2, 1, 8, 8, 6)


def test_product_stride2_gradient_with_the_se_affine(lib):
    """irse.hip's unit_bwd: d(u + q2) = dY * s[b][c] + r[b][c] on the LIVE pixels of the zero-stuffed image only, then conv2's gradient"""
    B, Ho, Wo, O, I = 2, 3, 5, 20, 8
    g = gen(11)
    w = spread((O, I, 3, 3), g, -2, 2) / math.sqrt(9 * I)
    dy = spread((B * Ho * Wo, O), g)
    s, r = torch.rand(B, O, generator=g), torch.randn(B, O, generator=g) * 0.1
    got, _, _ = precise_conv(lib, dy, w, None, 1, 1, B, Ho, Wo, op=R.P_AFFINE, p=s, q=r, pq_img=1, geo=2, what="s2 dgrad + SE affine")
    pre = R.expand_pq(s, 1, B, Ho * Wo, O) * dy.double() + R.expand_pq(r, 1, B, Ho * Wo, O)
    ref, _ = conv_reference(dy, w, None, B, Ho, Wo, 2, True, pre=pre)
    _, mag = conv_reference(dy, w, None, B, Ho, Wo, 2, True, pre=pre.abs())
    R.check_product(got[:, :I], ref, mag, 9 * R.split_kp(O), "product_dgrad s2+affine", MG)


def test_product_flatten_permutation(lib):
    """a Linear behind an NCHW flatten (perm_hw = 4 pixels, perm_c = 12 channels): NHWC activations against torch's flatten order"""
    O, hw, ch, M = 6, 4, 12, 5
    g = gen(12)
    w = spread((O, ch * hw, 1, 1), g, -2, 2) / math.sqrt(ch * hw)
    x = spread((M, hw, ch), g)                               # NHWC: (pixel, channel)
    got, _, _ = precise_conv(lib, x.reshape(M, hw * ch), w, None, 0, 0, 1, M, 1, perm=(hw, ch), what="flatten fwd")
    x_nchw = x.permute(0, 2, 1).reshape(M, ch * hw).double()
    w2 = w.reshape(O, ch * hw).double()
    R.check_product(got[:, :O], x_nchw @ w2.t(), x_nchw.abs() @ w2.abs().t(), R.split_kp(ch * hw), "product_fwd flatten", MG)
    dy = spread((M, O), g)
    ggot, _, _ = precise_conv(lib, dy, w, None, 1, 0, 1, M, 1, perm=(hw, ch), what="flatten dgrad")
    gref = (dy.double() @ w2).reshape(M, ch, hw).permute(0, 2, 1).reshape(M, hw * ch)
    gmag = (dy.double().abs() @ w2.abs()).reshape(M, ch, hw).permute(0, 2, 1).reshape(M, hw * ch)
    R.check_product(ggot, gref, gmag, R.split_kp(O), "product_dgrad flatten", MG)


def test_product_split_k_slabs_and_register_fold_agree(lib):
    """2048 -> 512 channels, 128 rows per image (canonical chunk: 6 of the 96 K-tiles).  Two images run as 16 split-K slabs, seventeen
    fold the same chunks in registers: each against fp64, each on the path it names, image 0 with the same bits on both paths."""
    O, I, per = 512, 2048, 128
    g = gen(13)
    w = spread((O, I, 1, 1), g, -2, 2) / math.sqrt(I)
    x = spread((17 * per, I), g)
    K = R.split_kp(I)
    assert lib.hedit_k_gemm_canonical_chunk(per * 4, O, K) == 6
    assert lib.hedit_k_gemm_plan_splits(2 * per, O, K, 6) == 16 and lib.hedit_k_gemm_plan_splits(17 * per, O, K, 6) == 1
    w64 = w.reshape(O, I).double()
    small, ck, sp = precise_conv(lib, x[:2 * per], w, None, 0, 0, 2, per, 1, what="split-K slabs")
    assert (ck, sp) == (6, 16), (ck, sp)
    R.check_product(small, x[:2 * per].double() @ w64.t(), x[:2 * per].double().abs() @ w64.abs().t(), K, "product_fwd split-K", MG)
    big, ck, sp = precise_conv(lib, x, w, None, 0, 0, 17, per, 1, what="register fold")
    assert (ck, sp) == (6, 1), (ck, sp)
    R.check_product(big, x.double() @ w64.t(), x.double().abs() @ w64.abs().t(), K, "product_fwd register-fold", MG)
    assert bits_equal(big[:2 * per], small), "the slab path and the in-register fold give different bits"


def test_product_is_batch_invariant(lib):
    """image 1 of a three-image call == its one-image call, bit for bit (3 x 3 and linear, forward and gradient)"""
    g = gen(14)
    for (O, I, k, mode, H, W) in ((5, 24, 3, 1, 6, 4), (10, 100, 1, 0, 37, 1), (6, 8, 3, 2, 8, 8)):
        w = spread((O, I, k, k), g, -2, 2) / math.sqrt(I * k * k)
        x = spread((3 * H * W, I), g)
        three, _, _ = precise_conv(lib, x, w, None, 0, mode, 3, H, W, what="B=3")
        one, _, _ = precise_conv(lib, x[H * W:2 * H * W], w, None, 0, mode, 1, H, W, what="B=1")
        m = one.shape[0]
        assert bits_equal(three[m:2 * m], one), f"forward mode {mode} depends on the batch"
        dy = spread((3 * H * W, O), g)
        three, _, _ = precise_conv(lib, dy, w, None, 1, min(mode, 1), 3, H, W, what="B=3 dgrad")
        one, _, _ = precise_conv(lib, dy[H * W:2 * H * W], w, None, 1, min(mode, 1), 1, H, W, what="B=1 dgrad")
        assert bits_equal(three[H * W:2 * H * W], one), f"gradient mode {mode} depends on the batch"


# ------------------------------------------------------------------------------------------------------------------ pnet: BatchNorm, act
@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("C", [5, 300])
def test_bn_helpers(lib, C, rep):
    """p = g / sqrt(v + eps): sum, square root, quotient (3 roundings); q = b - m p: a product and a sum more.
    fold_bias: q = (bias - m) p + b."""
    g = gen(C)
    ga, be, me, bias = (torch.randn(C, generator=g) for _ in range(4))
    va = torch.rand(C, generator=g) + 0.1
    eps = 1e-5
    d = [gi(t) for t in (ga, be, me, va, bias)]

    def call(p, q):
        _lib.check(lib.hedit_k_bn_affine(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), eps, ptr(p), ptr(q), C, rep, None))

    p, q = run2("bn_affine", [C * rep, C * rep], call)
    p64 = ga.double() / torch.sqrt(va.double() + float(torch.tensor(eps)))
    q64 = be.double() - me.double() * p64
    R.check_bound(p, p64.repeat(rep), 5 * U * p64.abs().repeat(rep), "bn_affine p", MG)
    R.check_bound(q, q64.repeat(rep), (7 * U * (be.double().abs() + (me.double() * p64).abs())).repeat(rep), "bn_affine q", MG)
    for r in range(1, rep):
        assert bits_equal(p[:C], p[r * C:(r + 1) * C]) and bits_equal(q[:C], q[r * C:(r + 1) * C])
    if rep == 1:
        for bb, bd in ((bias, d[4]), (None, None)):
            def call2(p, q):
                _lib.check(lib.hedit_k_bn_fold_bias(ptr(bd), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), eps, ptr(p), ptr(q), C, None))

            p2, q2 = run2("bn_fold_bias", [C, C], call2)
            b64 = bb.double() if bb is not None else torch.zeros(C, dtype=torch.float64)
            assert bits_equal(p2, p[:C])
            R.check_bound(q2, (b64 - me.double()) * p64 + be.double(),
                          8 * U * ((b64.abs() + me.double().abs()) * p64.abs() + be.double().abs()), "bn_fold_bias q", MG)


@pytest.mark.parametrize("op,with_q", [(R.P_PRELU, True), (R.P_PRELU, False), (R.P_RELU, True), (R.P_RELU, False)])
def test_act_is_exact(lib, op, with_q):
    C, rows = 20, 333
    g = gen(op)
    x, p, q = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), (torch.randn(C, generator=g) if with_q else None)
    xd, pd, qd = gi(x), gi(p), gi(q)
    (y,) = run2("act", [rows * C], lambda y: _lib.check(lib.hedit_k_act(ptr(xd), ptr(pd), ptr(qd), ptr(y), rows * C, C, op, None)))
    t = x + q if with_q else x
    want = torch.where(t > 0, t, p * t if op == R.P_PRELU else torch.zeros_like(t))
    assert bits_equal(y.cpu().view(rows, C), want)


def test_scale_cols_is_exact(lib):
    n, rows = 77, 9
    g = gen(1)
    x, p = torch.randn(rows, n, generator=g), torch.randn(n, generator=g)
    xd, pd = gi(x), gi(p)
    (y,) = run2("scale_cols", [rows * n], lambda y: _lib.check(lib.hedit_k_scale_cols(ptr(xd), ptr(pd), ptr(y), rows * n, n, None)))
    assert bits_equal(y.cpu().view(rows, n), x * p)


# ------------------------------------------------------------------------------------------------------------------ squeeze-excitation
def se_slabs(HW):
    n = max(1, min(32, HW // 64))
    per = (HW + n - 1) // n
    return n, per


@functools.lru_cache(maxsize=None)
def se_case(C, HW):
    g = gen(C * 1000 + HW)
    B, Rr = 2, C // 16
    return dict(B=B, R=Rr, u=torch.randn(B, HW, C, generator=g), bias=torch.randn(C, generator=g) * 0.5,
                w1=torch.randn(Rr, C, generator=g) / math.sqrt(C), w2=torch.randn(C, Rr, generator=g) / math.sqrt(Rr),
                dY=torch.randn(B, HW, C, generator=g))


def slab_sums(t, HW):
    """[B][HW][C] fp64 -> [B][nslab][C]"""
    n, per = se_slabs(HW)
    return torch.stack([t[:, s * per:min(HW, (s + 1) * per)].sum(1) for s in range(n)], 1)


def se_chain(lib, c, C, HW, B, img0=0):
    """the five kernels on images img0 .. img0 + B of the case, each checked on ITS OWN inputs; returns their outputs"""
    Rr = c["R"]
    n, per = se_slabs(HW)
    assert lib.hedit_k_se_nslab(HW) == n
    u, dY = c["u"][img0:img0 + B], c["dY"][img0:img0 + B]
    ud, dYd, bd, w1d, w2d = gi(u), gi(dY), gi(c["bias"]), gi(c["w1"]), gi(c["w2"])
    u64, b64, w1, w2, dY64 = u.double(), c["bias"].double(), c["w1"].double(), c["w2"].double(), dY.double()
    chain = (per + 3) // 4 + 3               # a thread's pixels, then the four partial sums of a block

    (part,) = run2("se_pool", [B * n * C], lambda o: _lib.check(lib.hedit_k_se_pool(ptr(ud), ptr(o), B, HW, C, None)))
    R.check_bound(part, slab_sums(u64, HW).reshape(-1), (chain + 2) * U * slab_sums(u64.abs(), HW).reshape(-1), f"se_pool C={C} HW={HW}", MG)

    partd = gi(part)

    def fc(h, s):
        _lib.check(lib.hedit_k_se_fc(ptr(partd), ptr(bd), ptr(w1d), ptr(w2d), ptr(h), ptr(s), B, HW, C, Rr, None))

    h, s = run2("se_fc", [B * Rr, B * C], fc)
    p64 = part.double().cpu().view(B, n, C)
    pool = p64.sum(1) / HW + b64                                           # slabs in order, / HW, + bias
    pre = pool @ w1.t()                                                    # per lane C / 64 products, six wave steps
    h64 = pre.clamp_min(0)
    a = h64 @ w2.t()
    s64 = torch.sigmoid(a)
    n_dot = C // 64 + 1 + 6 + 2

    def fc_bounds(e_part):
        """errors of h and s given the error of the slab sums handed in"""
        e_pool = (n + 4) * U * (p64.abs().sum(1) / HW + b64.abs()) + e_part.sum(1) / HW
        e_h = n_dot * U * (pool.abs() @ w1.abs().t()) + e_pool @ w1.abs().t()
        e_a = (Rr + 2) * U * (h64.abs() @ w2.abs().t()) + e_h @ w2.abs().t()
        # s = 1 / (1 + e^-a): d s = s (1 - s) (d a + the exponential's relative error), then a sum and a quotient
        return e_h, s64 * (1 - s64) * (e_a + R.EXP_REL(a)) + 3 * U * s64

    e_h, e_s = fc_bounds(torch.zeros_like(p64))
    R.check_bound(h, h64.reshape(-1), e_h.reshape(-1), f"se_fc_h C={C} HW={HW}", MG)
    R.check_bound(s, s64.reshape(-1), e_s.reshape(-1), f"se_fc_s C={C} HW={HW}", MG)

    # backward.  gs = d/ds of sum dY (u + b) s: autograd on the forward restatement
    sv = torch.ones(B, 1, C, dtype=torch.float64, requires_grad=True)
    (gfull,) = torch.autograd.grad(((u64 + b64) * sv * dY64).sum(), sv)
    (gpart,) = run2("se_bwd_reduce", [B * n * C], lambda o: _lib.check(lib.hedit_k_se_bwd_reduce(ptr(dYd), ptr(ud), ptr(bd), ptr(o), B, HW, C, None)))
    terms = dY64 * (u64 + b64)
    e_gpart = (chain + 4) * U * slab_sums(dY64.abs() * (u64.abs() + b64.abs()), HW)
    R.check_bound(gpart, slab_sums(terms, HW).reshape(-1), e_gpart.reshape(-1), f"se_bwd_reduce C={C} HW={HW}", MG)
    assert torch.allclose(slab_sums(terms, HW).sum(1), gfull.reshape(B, C), rtol=1e-12, atol=1e-12)

    # r = d/d(u pixels) through the pooled path, from the kept s and h (here: the kernel's own, as the executor hands them on)
    gpd, sd, hd = gi(gpart), gi(s), gi(h)
    (rb,) = run2("se_fc_bwd", [B * C], lambda o: _lib.check(lib.hedit_k_se_fc_bwd(ptr(gpd), ptr(sd), ptr(hd), ptr(w1d), ptr(w2d), ptr(o), B, C, Rr, HW, None)))
    g64 = gpart.double().cpu().view(B, n, C)
    gs = g64.sum(1)
    pool_l = pool.clone().requires_grad_(True)
    s_l = torch.sigmoid((pool_l @ w1.t()).clamp_min(0) @ w2.t())
    (gpool,) = torch.autograd.grad(s_l, pool_l, gs)
    r64 = gpool / HW
    dt = gs * s64 * (1 - s64)
    dh = (dt @ w2) * (h64 > 0)

    def bwd_bounds(e_g, e_s_in):
        """error of r given the errors of the gradient's slab sums and of the s it is differentiated at: d (s (1 - s)) = (1 - 2 s) d s"""
        e_dt = ((n + 5) * U * g64.abs().sum(1) + e_g.sum(1)) * s64 * (1 - s64) + gs.abs() * (1 - 2 * s64).abs() * e_s_in
        e_dh = (n_dot * U * (dt.abs() @ w2.abs()) + e_dt @ w2.abs()) * (h64 > 0)
        return ((Rr + 3) * U * (dh.abs() @ w1.abs()) + e_dh @ w1.abs()) / HW

    e_r = bwd_bounds(torch.zeros_like(g64), e_s)
    # a hidden unit whose pre-activation is within its error of 0 could be masked either way: none in these cases
    assert bool(((pre.abs() > e_h) | ((pre <= 0) & (h.double().cpu().view(B, Rr) == 0))).all())
    R.check_bound(rb, r64.reshape(-1), e_r.reshape(-1), f"se_fc_bwd C={C} HW={HW}", MG)
    # the same bounds with the upstream kernels' own errors handed on: what the chain as a whole may be off by
    e_part = (chain + 2) * U * slab_sums(u64.abs(), HW)
    _, e_s_all = fc_bounds(e_part)
    e_r_all = bwd_bounds(e_gpart, e_s_all)
    return dict(part=part, h=h, s=s, gpart=gpart, r=rb, e_s=e_s_all, e_r=e_r_all)


@pytest.mark.parametrize("HW", [49, 196, 784])
@pytest.mark.parametrize("C", [64, 80, 512])
def test_se_chain(lib, C, HW):
    """pool -> fc -> (gradient) reduce -> fc_bwd at 1, 3 and 12 slabs with ragged last slabs, every kernel on its own inputs; the chain
    against fp64 autograd of Y = (u + b) sigmoid(W2 relu(W1 mean(u + b))); image 1 alone gives the bits it has in the batch."""
    c = se_case(C, HW)
    out = se_chain(lib, c, C, HW, 2)
    # d/du of sum(Y dY) = dY s + r: the chain's s and r against autograd from the ORIGINAL inputs, with every stage's bound handed on
    u = c["u"].double().requires_grad_(True)
    b64, w1, w2, dY = c["bias"].double(), c["w1"].double(), c["w2"].double(), c["dY"].double()
    s_true = torch.sigmoid(((u + b64).mean(1) @ w1.t()).clamp_min(0) @ w2.t())
    Y = (u + b64) * s_true[:, None, :]
    (du,) = torch.autograd.grad((Y * dY).sum(), u)
    s_k, r_k = out["s"].double().cpu().view(2, 1, C), out["r"].double().cpu().view(2, 1, C)
    got = dY * s_k + r_k
    bound = dY.abs() * out["e_s"][:, None, :] + out["e_r"][:, None, :]
    R.check_bound(got.reshape(-1), du.reshape(-1), bound.reshape(-1), f"se_chain_du C={C} HW={HW}", MG)
    one = se_chain(lib, c, C, HW, 1, img0=1)
    n = se_slabs(HW)[0]
    for k, per_img in (("part", n * C), ("h", c["R"]), ("s", C), ("gpart", n * C), ("r", C)):
        assert bits_equal(out[k][per_img:2 * per_img], one[k]), f"{k}: image 1 depends on the batch"


@pytest.mark.parametrize("conv_sc", [False, True], ids=["identity", "conv"])
@pytest.mark.parametrize("stride", [1, 2])
def test_se_combine_and_unit_bwd_combine(lib, stride, conv_sc):
    """Y = (u + bias) s + shortcut: three dependent roundings (four with the shortcut's bias).  dX = p dxa + the shortcut's gradient on
    the stride grid: autograd of  sum(p X dxa) + sum(X[::stride] dsc)."""
    B, Ho, Wo, C = 2, 3, 5, 20
    g = gen(stride * 2 + conv_sc)
    u, s, bias = torch.randn(B, Ho, Wo, C, generator=g), torch.rand(B, C, generator=g), torch.randn(C, generator=g)
    sc, scb = torch.randn(B, Ho, Wo, C, generator=g), torch.randn(C, generator=g)
    X = torch.randn(B, Ho * stride, Wo * stride, C, generator=g)
    d = [gi(t) for t in (u, bias, s, sc if conv_sc else None, scb if conv_sc else None, None if conv_sc else X)]

    def call(Y):
        _lib.check(lib.hedit_k_se_combine(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(d[5]), stride, ptr(Y), B, Ho, Wo, C, None))

    (Y,) = run2("se_combine", [B * Ho * Wo * C], call)
    main = (u.double() + bias.double()) * s.double()[:, None, None, :]
    sh = sc.double() + scb.double() if conv_sc else X.double()[:, ::stride, ::stride]
    sh_mag = sc.double().abs() + scb.double().abs() if conv_sc else sh.abs()
    mag = (u.double().abs() + bias.double().abs()) * s.double()[:, None, None, :] + sh_mag
    R.check_bound(Y, (main + sh).reshape(-1), 6 * U * mag.reshape(-1), "se_combine", MG)
    H, W = Ho * stride, Wo * stride
    dxa, p, dsc = torch.randn(B, H, W, C, generator=g), torch.randn(C, generator=g), torch.randn(B, Ho, Wo, C, generator=g)
    e = [gi(t) for t in (dxa, p, dsc)]
    (dX,) = run2("unit_bwd_combine", [B * H * W * C],
                 lambda o: _lib.check(lib.hedit_k_unit_bwd_combine(ptr(e[0]), ptr(e[1]), ptr(e[2]), stride, ptr(o), B, H, W, C, None)))
    Xl = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad((p.double() * Xl * dxa.double()).sum() + (Xl[:, ::stride, ::stride] * dsc.double()).sum(), Xl)
    Xm = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
    (mg,) = torch.autograd.grad((p.double().abs() * Xm * dxa.double().abs()).sum() + (Xm[:, ::stride, ::stride] * dsc.double().abs()).sum(), Xm)
    R.check_bound(dX, ref.reshape(-1), 4 * U * mg.reshape(-1), "unit_bwd_combine", MG)


# ------------------------------------------------------------------------------------------------------------------ face pool, cosine head
@pytest.mark.parametrize("ldg", [3, 8])
def test_face_pool_and_its_gradient(lib, ldg):
    """adaptive_avg_pool2d(img[:, :, 35:223, 32:220], 112): windows of at most 3 x 3 pixels summed in order and divided (9 + 1
    roundings); the gradient sums at most 2 x 2 windows' quotients (4 + 1), zero outside the crop"""
    B = 2
    g = gen(ldg)
    img = torch.randn(B, 3, 256, 256, generator=g)
    imd = gi(img)
    (out,) = run2("face_pool", [B * 112 * 112 * 3], lambda o: _lib.check(lib.hedit_k_face_pool(ptr(imd), ptr(o), B, None)))
    ref = F.adaptive_avg_pool2d(img.double()[:, :, 35:223, 32:220], (112, 112))
    mag = F.adaptive_avg_pool2d(img.double().abs()[:, :, 35:223, 32:220], (112, 112))
    R.check_bound(out, ref.permute(0, 2, 3, 1).reshape(-1), 12 * U * mag.permute(0, 2, 3, 1).reshape(-1), "face_pool", MG)
    gr = torch.randn(B * 112 * 112, 3, generator=g)
    gd = gi2(gr, ldg)
    (dimg,) = run2("face_pool_bwd", [B * 3 * 256 * 256], lambda o: _lib.check(lib.hedit_k_face_pool_bwd(ptr(gd), ldg, ptr(o), B, None)))
    res = []
    for gg in (gr.double(), gr.double().abs()):
        il = torch.zeros(B, 3, 256, 256, dtype=torch.float64, requires_grad=True)
        (t,) = torch.autograd.grad(F.adaptive_avg_pool2d(il[:, :, 35:223, 32:220], (112, 112)), il, gg.reshape(B, 112, 112, 3).permute(0, 3, 1, 2))
        res.append(t.reshape(-1))
    R.check_bound(dimg, res[0], 7 * U * res[1], "face_pool_bwd", MG)
    outside = torch.ones(256, 256, dtype=torch.bool)
    outside[35:223, 32:220] = False
    assert bool((dimg.cpu().view(B, 3, 256, 256)[:, :, outside].view(torch.int32) == 0).all()), "gradient outside the crop is not exact zero"


@pytest.mark.parametrize("ref_stride", [0, 512])
def test_cos_head(lib, ref_stride):
    """f = raw + bias, e = f / |f|, e2 = e / |e|, loss = 1 - <e2, ref>, df = d(scale loss) / d raw through both normalisations (fp64
    autograd).  Relative roundings: f 1; |f|^2 two per thread + six wave steps + three partial sums = 11 (+1 squares) -> |f| 7;
    e 9; |e|^2 2 * 9 + 12 = 30 -> |e| 16; e2 26.  The dot product adds 12 on sum |e2 ref|; k = -scale / (|f| |e|) 25."""
    B, D, scale = 3, 512, 0.7
    g = gen(ref_stride)
    raw, bias = torch.randn(B, D, generator=g), torch.randn(D, generator=g) * 0.3
    ref = F.normalize(torch.randn(B if ref_stride else 1, D, generator=g), dim=1)
    rd, bd, fd = gi(raw), gi(bias), gi(ref)

    def call(feat, loss, df):
        _lib.check(lib.hedit_k_cos_head(ptr(rd), ptr(bd), ptr(fd), ref_stride, ptr(feat), ptr(loss), ptr(df), B, D, scale, None))

    feat, loss, df = run2("cos_head", [B * D, B, B * D], call)
    rl = raw.double().requires_grad_(True)
    f = rl + bias.double()
    e2 = F.normalize(f / f.norm(dim=1, keepdim=True), dim=1)
    r64 = ref.double().expand(B, D)
    cs = (e2 * r64).sum(1)
    (dref,) = torch.autograd.grad((scale * (1 - cs)).sum(), rl)
    e2, cs = e2.detach(), cs.detach()
    R.check_bound(feat, e2.reshape(-1), 26 * U * e2.abs().reshape(-1), "cos_head feat", MG)
    e_cs = 38 * U * (e2.abs() * r64.abs()).sum(1)
    R.check_bound(loss, 1 - cs, e_cs + U * (1 - cs).abs(), "cos_head loss", MG)
    k = scale / (f.detach().norm(dim=1, keepdim=True))          # |e| = 1
    inner = e_cs[:, None] * e2.abs() + cs.abs()[:, None] * 26 * U * e2.abs() + 2 * U * (r64.abs() + (cs[:, None] * e2).abs())
    R.check_bound(df, dref.reshape(-1), (k * inner + 26 * U * dref.abs()).reshape(-1), "cos_head df", MG)
    # features only (no reference): the same feat bits
    (feat2,) = run2("cos_head feat", [B * D], lambda o: _lib.check(lib.hedit_k_cos_head(ptr(rd), ptr(bd), None, 0, ptr(o), None, None, B, D, scale, None)))
    assert bits_equal(feat2, feat)


# ------------------------------------------------------------------------------------------------------------------ LPIPS pieces
def test_lpips_prep_and_its_gradient(lib):
    B, H, W = 2, 6, 10
    g = gen(3)
    img = torch.randn(B, 3, H, W, generator=g)
    shift, scale = [-0.030, -0.088, -0.188], [0.458, 0.448, 0.450]
    sh3, sc3 = (ctypes.c_float * 3)(*shift), (ctypes.c_float * 3)(*scale)
    sh64 = torch.tensor([float(v) for v in sh3], dtype=torch.float64).reshape(1, 3, 1, 1)
    sc64 = torch.tensor([float(v) for v in sc3], dtype=torch.float64).reshape(1, 3, 1, 1)
    imd = gi(img)
    (out,) = run2("lpips_prep", [B * H * W * 3], lambda o: _lib.check(lib.hedit_k_lpips_prep(ptr(imd), ptr(o), sh3, sc3, B, H, W, None)))
    il = img.double().requires_grad_(True)
    y = (il - sh64) / sc64
    R.check_bound(out, y.detach().permute(0, 2, 3, 1).reshape(-1), 4 * U * ((img.double().abs() + sh64.abs()) / sc64).permute(0, 2, 3, 1).reshape(-1),
                  "lpips_prep", MG)
    for ldg in (3, 8):
        gr = torch.randn(B * H * W, 3, generator=g)
        gd = gi2(gr, ldg)
        (dimg,) = run2("lpips_prep_bwd", [B * 3 * H * W], lambda o: _lib.check(lib.hedit_k_lpips_prep_bwd(ptr(gd), ldg, ptr(o), sc3, B, H, W, None)))
        (dref,) = torch.autograd.grad(y, il, gr.double().reshape(B, H, W, 3).permute(0, 3, 1, 2), retain_graph=True)
        R.check_bound(dimg, dref.reshape(-1), 3 * U * dref.abs().reshape(-1), f"lpips_prep_bwd ldg={ldg}", MG)


def maxpool(lib, z, B, H, W, C):
    zd = gi(z)
    n = B * (H // 2) * (W // 2) * C
    assert n % 4 == 0

    def call(zp, idx):
        _lib.check(lib.hedit_k_maxpool2(ptr(zd), ptr(zp), ptr(idx), B, H, W, C, None))

    zp, idx = run2("maxpool2", [n, n // 4], call, finite=False)
    return zp.cpu().view(B, H // 2, W // 2, C), idx.view(torch.uint8).cpu().view(B, H // 2, W // 2, C)


def maxpool_bwd(lib, gp, idx, add, B, H, W, C):
    gd, idd, ad = gi(gp), idx.contiguous().to(G.dev()), gi(add)
    (Gf,) = run2("maxpool2_bwd", [B * H * W * C], lambda o: _lib.check(lib.hedit_k_maxpool2_bwd(ptr(gd), ptr(idd), ptr(ad), ptr(o), B, H, W, C, None)))
    return Gf.cpu().view(B, H, W, C)


def test_maxpool2_random(lib):
    """values, winners and the scattered gradient against torch (no ties in random data); data movement and one sum: exact"""
    B, H, W, C = 2, 6, 10, 12
    g = gen(4)
    z = torch.randn(B, H, W, C, generator=g)
    zp, idx = maxpool(lib, z, B, H, W, C)
    zl = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want, widx = F.max_pool2d(zl, 2, return_indices=True)
    assert bits_equal(zp, want.detach().permute(0, 2, 3, 1))
    wy, wx = widx // W, widx % W
    assert torch.equal(idx.long(), ((wy % 2) * 2 + wx % 2).permute(0, 2, 3, 1))
    gp, add = torch.randn(B, H // 2, W // 2, C, generator=g), torch.randn(B, H, W, C, generator=g)
    (gz,) = torch.autograd.grad(want, zl, gp.permute(0, 3, 1, 2))
    gz = gz.permute(0, 2, 3, 1)
    assert bits_equal(maxpool_bwd(lib, gp, idx, None, B, H, W, C), 0.0 + gz)
    assert bits_equal(maxpool_bwd(lib, gp, idx, add, B, H, W, C), add + gz)


def test_maxpool2_ties(lib):
    """constant windows: the recorded winner is a maximum, exactly one pixel per window receives the gradient, `add` passes through"""
    B, H, W, C = 1, 4, 8, 8
    g = gen(5)
    z = torch.randn(B, H // 2, W // 2, C, generator=g).repeat_interleave(2, 1).repeat_interleave(2, 2)
    z[0, 0, 0:2, 0] = torch.tensor([1.0, 2.0])         # one window with a unique maximum among equals elsewhere
    zp, idx = maxpool(lib, z, B, H, W, C)
    win = z.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    assert bits_equal(zp, win.max(-1).values)
    assert bool((idx < 4).all()) and bits_equal(torch.gather(win, -1, idx.long()[..., None])[..., 0], zp)
    gp = torch.rand(B, H // 2, W // 2, C, generator=g) + 1.0
    add = torch.randn(B, H, W, C, generator=g)
    G0 = maxpool_bwd(lib, gp, idx, None, B, H, W, C)
    gw = G0.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    assert bool(((gw != 0).sum(-1) == 1).all()) and bits_equal(gw.sum(-1), gp)
    assert bits_equal(torch.gather(gw, -1, idx.long()[..., None])[..., 0], gp)
    assert bits_equal(maxpool_bwd(lib, gp, idx, add, B, H, W, C), add + G0)


@pytest.mark.parametrize("C", [64, 512])
def test_lpips_head(lib, C):
    """F = relu(z + bias), Fn = F / (|F| + 1e-10).  |F|^2: C / 64 squares per lane + six wave steps (n <= 15) -> |F| 8.5, + eps 9.5,
    Fn 11.5 roundings.  d = sum w (Fn - src)^2 and dF = d(gscale sum d) / dF (fp64 autograd on the leaf F) with the bounds propagated
    term by term below.  A pixel whose features are all zero takes dF = g / n (the norm's own gradient is dropped there)."""
    B, HW = 2, 5
    g = gen(C)
    z, bias = torch.randn(B * HW, C, generator=g), torch.randn(C, generator=g) * 0.2
    w = torch.rand(C, generator=g)
    gscale = 0.37
    n_ss = C // 64 + 7
    zd, bd, wd = gi(z), gi(bias), gi(w)
    (fn,) = run2("lpips_head fn", [B * HW * C],
                 lambda o: _lib.check(lib.hedit_k_lpips_head(ptr(zd), ptr(bd), None, 0, None, ptr(o), None, None, B, HW, C, gscale, None)))
    F64 = (z.double() + bias.double()).clamp_min(0)
    Fn = F64 / (F64.norm(dim=1, keepdim=True) + 1e-10)
    R.check_bound(fn, Fn.reshape(-1), 12 * U * Fn.reshape(-1), f"lpips_head_fn C={C}", MG)
    src_img = torch.rand(B, HW, C, generator=g) * 0.1
    for name, src, stride, zero_pixel in (("shared", src_img[:1], 0, False), ("per-image", src_img, HW * C, False), ("zero pixel", src_img, HW * C, True)):
        zz = z.clone()
        if zero_pixel:
            zz[3] = -bias - 1.0                     # every pre-activation of pixel 3 negative
        zzd, sd = gi(zz), gi(src)

        def call(dpix, dF):
            _lib.check(lib.hedit_k_lpips_head(ptr(zzd), ptr(bd), ptr(sd), stride, ptr(wd), None, ptr(dpix), ptr(dF), B, HW, C, gscale, None))

        dpix, dF = run2(f"lpips_head {name}", [B * HW, B * HW * C], call)
        Fl = (zz.double() + bias.double()).clamp_min(0).requires_grad_(True)
        nrm = (Fl * Fl).sum(1, keepdim=True).sqrt()
        s64 = src.double().expand(B, HW, C).reshape(B * HW, C)
        live = (nrm.detach() > 0).reshape(-1)
        Fn = Fl / (nrm + 1e-10)
        dfv = Fn - s64
        d = (w.double() * dfv * dfv).sum(1)
        (dref,) = torch.autograd.grad(gscale * d[live].sum(), Fl)
        Fd, Fn, dfv, nrm = Fl.detach(), Fn.detach(), dfv.detach(), nrm.detach()
        nn_ = nrm + 1e-10
        gvec = 2 * w.double() * dfv * gscale
        dref[~live] = (gvec / nn_)[~live]
        w64 = w.double()
        e_df = 12 * U * Fn + U * dfv.abs()
        R.check_bound(dpix, d.detach(), (w64 * (2 * dfv.abs() * e_df + (n_ss + 4) * U * dfv * dfv)).sum(1), f"lpips_head_d C={C} {name}", MG)
        e_g = 2 * w64 * gscale * e_df + 3 * U * gvec.abs()
        e_gf = (e_g * Fd + (n_ss + 3) * U * gvec.abs() * Fd).sum(1, keepdim=True)
        k2 = torch.where(nrm > 0, (gvec * Fd).sum(1, keepdim=True) / (nrm * nn_ * nn_).clamp_min(1e-300), torch.zeros_like(nrm))
        e_k2 = torch.where(nrm > 0, e_gf / (nrm * nn_ * nn_).clamp_min(1e-300) + 32 * U * k2.abs(), torch.zeros_like(nrm))
        e_dF = e_g / nn_ + 11 * U * (gvec / nn_).abs() + Fd * e_k2 + 2 * U * (Fd * k2).abs() + U * ((gvec / nn_).abs() + (Fd * k2).abs())
        R.check_bound(dF, dref.reshape(-1), e_dF.reshape(-1), f"lpips_head_dF C={C} {name}", MG)
        # without dF: the same dpix bits
        (dpix2,) = run2(f"lpips_head {name} no dF", [B * HW],
                        lambda o: _lib.check(lib.hedit_k_lpips_head(ptr(zzd), ptr(bd), ptr(sd), stride, ptr(wd), None, ptr(o), None, B, HW, C, gscale, None)))
        assert bits_equal(dpix2, dpix)


@pytest.mark.parametrize("HW", [1, 49, 3000])
def test_lpips_reduce(lib, HW):
    """mean over the pixels: ceil(HW / 256) terms per thread, six wave steps, three partial sums, the quotient (and the running sum)"""
    B = 3
    g = gen(HW)
    dpix, acc0 = torch.rand(B, HW, generator=g), torch.randn(B, generator=g)
    dd = gi(dpix)
    n = (HW + 255) // 256 + 10
    mean = dpix.double().mean(1)
    (acc,) = run2("lpips_reduce first", [B], lambda o: _lib.check(lib.hedit_k_lpips_reduce(ptr(dd), ptr(o), B, HW, 1, None)))
    R.check_bound(acc, mean, (n + 2) * U * mean, f"lpips_reduce HW={HW} first", MG)

    def call(o):
        o.copy_(acc0.to(G.dev()))
        _lib.check(lib.hedit_k_lpips_reduce(ptr(dd), ptr(o), B, HW, 0, None))

    (acc2,) = run2("lpips_reduce add", [B], call)
    R.check_bound(acc2, acc0.double() + mean, (n + 2) * U * mean + U * (acc0.double().abs() + mean), f"lpips_reduce HW={HW} add", MG)


# ------------------------------------------------------------------------------------------------------------------ encoder kernels
def test_patchify_both_directions(lib):
    B, Rr, p = 2, 12, 4
    P = Rr // p
    img = torch.randn(B, 3, Rr, Rr, generator=gen(6))
    imd = gi(img)
    n = B * P * P * 3 * p * p
    (X,) = run2("patchify", [n], lambda o: _lib.check(lib.hedit_k_enc_patchify(ptr(imd), ptr(o), B, Rr, p, 0, None)))
    want = F.unfold(img, p, stride=p).permute(0, 2, 1).reshape(B * P * P, 3 * p * p)      # column = (c, ky, kx)
    assert bits_equal(X.cpu().view(B * P * P, 3 * p * p), want)
    Xd = gi(want)
    (back,) = run2("patchify bwd", [B * 3 * Rr * Rr], lambda o: _lib.check(lib.hedit_k_enc_patchify(ptr(o), ptr(Xd), B, Rr, p, 1, None)))
    assert bits_equal(back.cpu().view(B, 3, Rr, Rr), img)


@pytest.mark.parametrize("with_bias", [False, True])
def test_tokens_gather_drop_cls_add_bias_res(lib, with_bias):
    B, L, W = 3, 6, 20
    g = gen(7 + with_bias)
    E, cb, cls, pos = torch.randn(B * (L - 1), W, generator=g), torch.randn(W, generator=g), torch.randn(W, generator=g), torch.randn(L, W, generator=g)
    d = [gi(t) for t in (E, cb if with_bias else None, cls, pos)]
    (T,) = run2("tokens", [B * L * W], lambda o: _lib.check(lib.hedit_k_enc_tokens(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(o), B, L, W, None)))
    body = E.view(B, L - 1, W) + cb if with_bias else E.view(B, L - 1, W)
    want = torch.cat([cls.expand(B, 1, W), body], 1) + pos
    T = T.cpu().view(B, L, W)
    assert bits_equal(T, want)
    Td = gi(T)
    idx = torch.tensor([4, -3, 99], dtype=torch.int32)
    for ix, rows in ((idx.to(G.dev()), [4, 0, L - 1]), (None, [0, 0, 0])):
        (Rw,) = run2("gather_rows", [B * W], lambda o: _lib.check(lib.hedit_k_enc_gather_rows(ptr(Td), ptr(ix), ptr(o), B, L, W, None)))
        assert bits_equal(Rw.cpu().view(B, W), torch.stack([T[b, rows[b]] for b in range(B)]))
    (dE,) = run2("drop_cls", [B * (L - 1) * W], lambda o: _lib.check(lib.hedit_k_vit_drop_cls(ptr(Td), ptr(o), B, L, W, None)))
    assert bits_equal(dE.cpu().view(B, L - 1, W), T[:, 1:])
    raw, res = torch.randn(B * L, W, generator=g), torch.randn(B * L, W, generator=g)
    rd, sd, bd = gi(raw), gi(res), gi(cb)
    (o1,) = run2("add_bias_res", [B * L * W], lambda o: _lib.check(lib.hedit_k_enc_add_bias_res(ptr(rd), ptr(bd), ptr(sd), ptr(o), B * L * W, W, None)))
    assert bits_equal(o1.cpu().view(B * L, W), res + raw + cb)
    (o2,) = run2("add_bias", [B * L * W], lambda o: _lib.check(lib.hedit_k_enc_add_bias_res(ptr(rd), ptr(bd), None, ptr(o), B * L * W, W, None)))
    assert bits_equal(o2.cpu().view(B * L, W), raw + cb)


def ln_bounds(x, g, b, eps):
    """fp64 LayerNorm of x [rows][W] with the error of the fp32 kernel: mean = (ceil(W / 64) per-lane terms + six wave steps) / W;
    d = x - mean; var likewise over d^2; rstd = rsqrt(var + eps) (2 ulp); y = d rstd g + b (three more)"""
    W = x.shape[1]
    n = (W + 63) // 64 + 7
    mean = x.mean(1, keepdim=True)
    e_mean = (n + 2) * U * x.abs().mean(1, keepdim=True)
    dd = x - mean
    e_d = e_mean + U * dd.abs()
    var = (dd * dd).mean(1, keepdim=True)
    e_var = (2 * dd.abs() * e_d).mean(1, keepdim=True) + (n + 3) * U * var
    rstd = 1 / torch.sqrt(var + eps)
    e_rstd = rstd * (0.5 * e_var / (var + eps) + 4 * U)
    y = dd * rstd * g + b
    e_y = g.abs() * (e_d * rstd + dd.abs() * e_rstd) + 4 * U * ((dd * rstd * g).abs() + b.abs())
    return dict(mean=mean, rstd=rstd, y=y, e_mean=e_mean, e_rstd=e_rstd, e_y=e_y, n=n)


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("W", [64, 100, 128])
def test_layernorm_forward_statistics_and_backward(lib, W, with_add):
    """nine rows (ragged against four rows per block).  Forward with and without the statistics output (same y bits), statistics
    against fp64; the backward from those statistics against fp64 autograd of F.layer_norm."""
    rows, eps = 9, 1e-5
    g = gen(W)
    x = torch.randn(rows, W, generator=g) * 2 + 0.7
    ga, be, dy, add = torch.randn(W, generator=g), torch.randn(W, generator=g), torch.randn(rows, W, generator=g), torch.randn(rows, W, generator=g)
    xd, gd, bd, dyd, ad = gi(x), gi(ga), gi(be), gi(dy), gi(add if with_add else None)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    y, st = run2("enc_ln", [rows * W, rows * 2], lambda y, s: _lib.check(lib.hedit_k_enc_ln(ptr(xd), ptr(gd), ptr(bd), ptr(y), ptr(s), rows, W, eps, None)))
    (y0,) = run2("enc_ln no stats", [rows * W], lambda y: _lib.check(lib.hedit_k_enc_ln(ptr(xd), ptr(gd), ptr(bd), ptr(y), None, rows, W, eps, None)))
    assert bits_equal(y, y0)
    r = ln_bounds(x.double(), ga.double(), be.double(), eps32)
    R.check_bound(y, r["y"].reshape(-1), r["e_y"].reshape(-1), f"enc_ln_y W={W}", MG)
    st = st.cpu().view(rows, 2)
    R.check_bound(st[:, 0], r["mean"].reshape(-1), r["e_mean"].reshape(-1), f"enc_ln_mean W={W}", MG)
    R.check_bound(st[:, 1], r["rstd"].reshape(-1), r["e_rstd"].reshape(-1), f"enc_ln_rstd W={W}", MG)
    # backward: dx = add + rstd (t - mean(t) - xh mean(t xh)), t = dy g, xh = (x - mean) rstd, from the kernel's own statistics
    std = gi(st)
    (dx,) = run2("vit_ln_bwd", [rows * W], lambda o: _lib.check(lib.hedit_k_vit_ln_bwd(ptr(xd), ptr(dyd), ptr(gd), ptr(std), ptr(ad), ptr(o), rows, W, None)))
    xl = x.double().requires_grad_(True)
    (dref,) = torch.autograd.grad(F.layer_norm(xl, (W,), ga.double(), be.double(), eps32), xl, dy.double())
    n = r["n"]
    rstd, xh = r["rstd"], (x.double() - r["mean"]) * r["rstd"]
    e_xh = rstd * r["e_mean"] + xh.abs() * r["e_rstd"] / rstd + 3 * U * xh.abs()
    t = dy.double() * ga.double()
    a, c = t.mean(1, keepdim=True), (t * xh).mean(1, keepdim=True)
    e_a = (n + 3) * U * t.abs().mean(1, keepdim=True)
    e_c = (t.abs() * e_xh).mean(1, keepdim=True) + (n + 4) * U * (t * xh).abs().mean(1, keepdim=True)
    S = rstd * (t.abs() + a.abs() + (xh * c).abs())
    e_v = rstd * (e_a + e_xh * c.abs() + xh.abs() * e_c) + (t - a - xh * c).abs() * r["e_rstd"] + 6 * U * S
    ref = dref + (add.double() if with_add else 0)
    R.check_bound(dx, ref.reshape(-1), (e_v + U * ((add.double().abs() if with_add else 0) + S)).reshape(-1), f"vit_ln_bwd W={W}", MG)


# ------------------------------------------------------------------------------------------------------------------ ViT attention
HEADS, HD = 2, 64


@functools.lru_cache(maxsize=None)
def attn_case(L):
    """three images; fp64 forward and autograd gradients with the first-order error bounds of the fp32 kernels (docstrings of the tests)"""
    B, Wd = 3, HEADS * HD
    g = gen(L)
    qkv = torch.randn(B * L, 3 * Wd, generator=g)
    bias = torch.randn(3 * Wd, generator=g) * 0.5
    dA = torch.randn(B * L, Wd, generator=g)
    scale = 0.125
    leaf = qkv.double().requires_grad_(True)
    t = (leaf + bias.double()).view(B, L, 3, HEADS, HD).permute(2, 0, 3, 1, 4)       # [3][B][h][L][d]
    q, k, v = t[0], t[1], t[2]
    s = (q * scale) @ k.transpose(-1, -2)
    P = torch.softmax(s, -1)
    A = (P @ v).permute(0, 2, 1, 3).reshape(B * L, Wd)
    lse = torch.logsumexp(s, -1)
    (dqkv,) = torch.autograd.grad(A, leaf, dA.double())
    q, k, v, s, P, A, lse = (x.detach() for x in (q, k, v, s, P, A, lse))
    qs = q * scale
    n_o = L // 2 + 4                                   # two interleaved chains over the keys, folded at the end
    n_s = (L + 63) // 64 + 6
    # scores: 64 products in one chain, operands rounded once (bias) or twice (bias, scale)
    e_s = 69 * U * (qs.abs() @ k.abs().transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    rho = e_s + U * (s - m).abs() + R.EXP_REL(s - m)              # relative error of exp(s - max); the max's own error cancels in the ratio
    rho_sum = (P * rho).sum(-1, keepdim=True) + (n_s + 2) * U
    e_A = (P * (rho + rho_sum + (n_o + 4) * U)) @ v.abs()
    e_lse = rho_sum[..., 0] + 4 * U * (lse - m[..., 0]).abs() + U * lse.abs()          # d lse = sum_j P_j d s_j; fast log; m + log
    # backward from fp32-rounded A and lse
    dAh = dA.double().view(B, L, HEADS, HD).permute(0, 2, 1, 3)
    Ah = A.view(B, L, HEADS, HD).permute(0, 2, 1, 3)
    D = (dAh * Ah).sum(-1, keepdim=True)
    e_D = 10 * U * (dAh.abs() * Ah.abs()).sum(-1, keepdim=True)
    rho_b = e_s + U * lse.abs()[..., None] + U * (s - lse[..., None]).abs() + R.EXP_REL(s - lse[..., None])
    dP = dAh @ v.transpose(-1, -2)
    e_dP = 67 * U * (dAh.abs() @ v.abs().transpose(-1, -2))
    ds = P * (dP - D)
    e_ds = P * (rho_b * (dP - D).abs() + e_dP + e_D + 2 * U * (dP.abs() + D.abs()))
    e_dq = scale * (e_ds @ k.abs() + (n_o + 4) * U * (ds.abs() @ k.abs()))
    e_dv = (P * (rho_b + (n_o + 3) * U)).transpose(-1, -2) @ dAh.abs()
    e_dk = e_ds.transpose(-1, -2) @ qs.abs() + (n_o + 5) * U * (ds.abs().transpose(-1, -2) @ qs.abs())

    def rows(x):      # [B][h][L][d] -> [B L][h d]
        return x.permute(0, 2, 1, 3).reshape(B * L, Wd)

    e_dqkv = torch.cat([rows(e_dq), rows(e_dk), rows(e_dv)], 1)
    return dict(B=B, qkv=qkv, bias=bias, dA=dA, A=A, lse=lse, dqkv=dqkv, e_A=rows(e_A), e_lse=e_lse, e_dqkv=e_dqkv)


def attn_fwd(lib, c, L, B, slices):
    Wd = HEADS * HD
    qd, bd = gi(c["qkv"][:B * L]), gi(c["bias"])

    def call(A, lse):
        _lib.check(lib.hedit_k_vit_attn_fwd(ptr(qd), ptr(bd), ptr(A), ptr(lse), B, L, HEADS, slices, None))

    A, lse = run2(f"vit_attn_fwd L={L} B={B} slices={slices}", [B * L * Wd, B * HEADS * L], call)
    return A.cpu().view(B * L, Wd), lse.cpu().view(B, HEADS, L)


def attn_bwd(lib, c, L, B, slices):
    Wd = HEADS * HD
    qd, bd, Ad = gi(c["qkv"][:B * L]), gi(c["bias"]), gi(c["A"][:B * L].float())
    dAd, ld = gi(c["dA"][:B * L]), gi(c["lse"][:B].float())

    def call(o):
        _lib.check(lib.hedit_k_vit_attn_bwd(ptr(qd), ptr(bd), ptr(Ad), ptr(dAd), ptr(ld), ptr(o), B, L, HEADS, slices, None))

    (o,) = run2(f"vit_attn_bwd L={L} B={B} slices={slices}", [B * L * 3 * Wd], call)
    return o.cpu().view(B * L, 3 * Wd)


@pytest.mark.parametrize("L", [9, 17, 197, 200])
def test_vit_attention_forward(lib, L):
    """A and lse against fp64 at 1, 2 and 4 slices (the slice tails end in a clamped duplicate row; L = 200 is LMAX) and B = 1 / 3:
    identical bits whatever the slice count and the batch.  Bound: the 64-term score chains, exp(s - max) with the fast exponential,
    the key sums in two interleaved chains of L / 2, the quotient; lse adds the fast logarithm."""
    c = attn_case(L)
    A, lse = attn_fwd(lib, c, L, 3, 1)
    R.check_bound(A.reshape(-1), c["A"].reshape(-1), c["e_A"].reshape(-1), f"vit_attn_A L={L}", MG)
    R.check_bound(lse.reshape(-1), c["lse"].reshape(-1), c["e_lse"].reshape(-1), f"vit_attn_lse L={L}", MG)
    for slices in (2, 4, 0):
        A2, lse2 = attn_fwd(lib, c, L, 3, slices)
        assert bits_equal(A2, A) and bits_equal(lse2, lse), f"slices={slices} changes the bits"
    for slices in (1, 4):
        A1, lse1 = attn_fwd(lib, c, L, 1, slices)
        assert bits_equal(A1, A[:L]) and bits_equal(lse1, lse[:1]), f"B=1 slices={slices}: image 0 depends on the batch"


@pytest.mark.parametrize("L", [9, 17, 197, 200])
def test_vit_attention_backward(lib, L):
    """dq, dk, dv (dqkv [B L][3W]) against fp64 autograd of softmax(scale q k^T) v, from the fp32-rounded A and lse of the fp64
    forward; identical bits whatever the slice count and the batch"""
    c = attn_case(L)
    d = attn_bwd(lib, c, L, 3, 1)
    Wd = HEADS * HD
    for name, lo in (("dq", 0), ("dk", Wd), ("dv", 2 * Wd)):
        R.check_bound(d[:, lo:lo + Wd].reshape(-1), c["dqkv"][:, lo:lo + Wd].reshape(-1), c["e_dqkv"][:, lo:lo + Wd].reshape(-1),
                      f"vit_attn_{name} L={L}", MG)
    for slices in (2, 4, 0):
        assert bits_equal(attn_bwd(lib, c, L, 3, slices), d), f"slices={slices} changes the bits"
    for slices in (1, 4):
        assert bits_equal(attn_bwd(lib, c, L, 1, slices), d[:L]), f"B=1 slices={slices}: image 0 depends on the batch"


def test_vit_gram_bwd(lib):
    """dT = d(scale |F^T F - Gref|_F) / dF behind a zero class row: autograd; the kernel scales F R (handed in fp32) by 2 scale / |R|"""
    L, W, scale = 7, 20, 0.3
    g = gen(8)
    Fm = torch.randn(L - 1, W, generator=g, dtype=torch.float64).requires_grad_(True)
    Gref = torch.randn(W, W, generator=g, dtype=torch.float64)
    Gref = Gref + Gref.t()
    Rm = Fm.t() @ Fm - Gref
    (dF,) = torch.autograd.grad(scale * Rm.norm(), Fm)
    FR, nrm = (Fm @ Rm).detach().float(), Rm.norm().detach().float().reshape(1)
    fd, nd = gi(FR), gi(nrm)
    (dT,) = run2("vit_gram_bwd", [L * W], lambda o: _lib.check(lib.hedit_k_vit_gram_bwd(ptr(fd), ptr(nd), ptr(o), L, W, scale, None)))
    dT = dT.cpu().view(L, W)
    assert bool((dT[0].view(torch.int32) == 0).all())
    R.check_bound(dT[1:].reshape(-1), dF.reshape(-1), 7 * U * dF.abs().reshape(-1), "vit_gram_bwd", MG)
    zd = gi(torch.zeros(1))
    (dT0,) = run2("vit_gram_bwd zero norm", [L * W], lambda o: _lib.check(lib.hedit_k_vit_gram_bwd(ptr(fd), ptr(zd), ptr(o), L, W, scale, None)))
    assert bool((dT0 == 0).all())          # 0 * F R: zeros of either sign
