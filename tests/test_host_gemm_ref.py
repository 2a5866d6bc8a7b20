"""CPU: the pointwise GEMM reference of tests/helpers/gemm_ref.py (used by tests/test_gpu_gemm_paths.py) is right and tight enough.

The row-sampled convolution reference equals F.conv2d in float64 in all three modes, and the comparator passes a result computed the way
the kernels compute it (fp32 accumulation of the storage-rounded operands, bf16(acc + bias), + residual rounded again) while it rejects
each of the faults a tiled kernel makes: a block that misses one K-tile, a conv row read from the neighbouring image row, a bias missing
on the ragged last column tile, a residual row shifted by one, a block written transposed."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import gemm_ref as R

DTYPES = [torch.bfloat16, torch.float16]


def _kernel_like(a, W, bias, res, dtype):
    """fp32 accumulation of the (storage-rounded) operands, then the epilogue's two roundings"""
    acc = a.float() @ W.float().t()
    if bias is not None:
        acc = acc + bias.float()
    out = acc.to(dtype)
    if res is not None:
        out = (out.float() + res.float()).to(dtype)
    return out


def _linear(M, N, K, dtype, seed, bias=True, res=False):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g).to(dtype) if res else None
    return A, W, b, r


def _ref(A, W, b, r, rows=None, mode=0, conv=None):
    M = A.shape[0] if mode == 0 else conv[0] * conv[4] * conv[5]
    rows = torch.arange(M) if rows is None else rows
    dot, mag = R.contract(R.rows_operand(A, rows, mode, conv), W)
    return R.reference(dot, mag, b, None if r is None else r[rows])


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_conv_rows_match_conv2d(mode):
    B, Hin, Win, Cin, N = 2, 5, 7, 3, 4
    g = torch.Generator().manual_seed(mode)
    x = torch.randn(B, Hin, Win, Cin, generator=g, dtype=torch.float64)
    w4 = torch.randn(N, Cin, 3, 3, generator=g, dtype=torch.float64)
    Wp = w4.permute(0, 2, 3, 1).reshape(N, 9 * Cin)          # the kernels' packed layout: k = (ky * 3 + kx) * Cin + ci
    xr = x.permute(0, 3, 1, 2)
    if mode == 1:
        want = F.conv2d(xr, w4, padding=1)
    elif mode == 2:
        want = F.conv2d(xr, w4, stride=2, padding=1)
    else:
        want = F.conv2d(F.interpolate(xr, scale_factor=2.0, mode="nearest"), w4, padding=1)
    Hout, Wout = R.conv_out_hw(mode, Hin, Win)
    assert want.shape[2:] == (Hout, Wout)
    want = want.permute(0, 2, 3, 1).reshape(-1, N)
    rows = torch.arange(B * Hout * Wout)                     # every row: the first and last image row of both images included
    dot, _ = R.contract(R.conv_rows(x, rows, mode, Hout, Wout), Wp)
    assert torch.allclose(dot, want, rtol=0, atol=1e-12)
    # a sample in any order gives the same rows
    sub = torch.tensor([B * Hout * Wout - 1, 0, Wout, Hout * Wout - 1])
    dot_s, _ = R.contract(R.conv_rows(x, sub, mode, Hout, Wout), Wp)
    assert torch.allclose(dot_s, want[sub], rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_clean_result_passes_and_a_missing_k_tile_is_rejected(dtype):
    M, N, K = 32, 64, 11520
    A, W, b, _ = _linear(M, N, K, dtype, seed=1)
    ref, pre, acc = _ref(A, W, b, None)
    got = _kernel_like(A, W, b, None, dtype)
    R.check_pointwise(got, ref, pre, acc, K, dtype, what="clean")
    # the accumulation term: the fp32 sum itself (before the output rounding) stays well inside c sqrt(K) 2^-24 sum|a w|
    acc32 = (A.float() @ W.float().t() + b).double()
    assert float(((acc32 - ref).abs() / (R.C_ACC * math.sqrt(K) * 2.0 ** -24 * acc)).max()) < 0.5
    # one 16 x 16 block misses K-tile 97 (64 of 11520 products: ~0.07 per element)
    bad = got.clone()
    r0, c0, kt = 16, 48, 97
    ks = slice(kt * 64, (kt + 1) * 64)
    part = A[r0:r0 + 16, ks].float() @ W[c0:c0 + 16, ks].float().t()
    bad[r0:r0 + 16, c0:c0 + 16] = (got[r0:r0 + 16, c0:c0 + 16].float() - part).to(dtype)
    with pytest.raises(AssertionError, match=r"worst at row (1[6-9]|2\d|3[01]), column (4[89]|5\d|6[0-3]) \(tile \(0, 0\)\)"):
        R.check_pointwise(bad, ref, pre, acc, K, dtype, tile=(256, 128), what="K-tile dropped")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_conv_row_from_the_neighbouring_image_row_is_rejected(dtype):
    B, H, Cin, N = 2, 8, 64, 32
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, H, H, Cin, generator=g).to(dtype)
    W = (torch.randn(N, 9 * Cin, generator=g) / math.sqrt(9 * Cin)).to(dtype)
    b = torch.randn(N, generator=g)
    conv = (B, H, H, Cin, H, H)
    rows = R.sample_rows(B * H * H, n_random=16, image=H * H, Wout=H)
    ref, pre, acc = _ref(x.reshape(-1, Cin), W, b, None, rows, mode=1, conv=conv)
    full = torch.arange(B * H * H)
    got = _kernel_like(R.conv_rows(x, full, 1, H, H), W, b, None, dtype)
    R.check_pointwise(got[rows], ref, pre, acc, 9 * Cin, dtype, rows=rows, what="clean conv")
    # image 1, output row 7 (the last) computed from output row 6's pixels
    bad = got.clone()
    y0 = H * H + 7 * H
    bad[y0:y0 + H] = got[y0 - H:y0]
    with pytest.raises(AssertionError, match=r"worst at row 12[0-7],"):
        R.check_pointwise(bad[rows], ref, pre, acc, 9 * Cin, dtype, rows=rows, what="row from the neighbouring row")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_bias_missing_on_the_ragged_column_tile_is_rejected(dtype):
    M, N, K = 64, 200, 192                               # 128-column tiles: the last one holds columns 128 .. 199
    A, W, b, r = _linear(M, N, K, dtype, seed=3, res=True)
    ref, pre, acc = _ref(A, W, b, r)
    got = _kernel_like(A, W, b, r, dtype)
    R.check_pointwise(got, ref, pre, acc, K, dtype, what="clean, residual")
    b_bad = b.clone()
    b_bad[128:] = 0
    bad = _kernel_like(A, W, b_bad, r, dtype)
    with pytest.raises(AssertionError, match=r"column (1[2-9]\d) \(tile \(\d+, 1\)\)"):
        R.check_pointwise(bad, ref, pre, acc, K, dtype, tile=(256, 128), what="bias missing")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_residual_row_shifted_by_one_is_rejected(dtype):
    M, N, K = 64, 160, 640
    A, W, b, r = _linear(M, N, K, dtype, seed=4, res=True)
    ref, pre, acc = _ref(A, W, b, r)
    r_bad = r.clone()
    r_bad[40] = r[41]
    bad = _kernel_like(A, W, b, r_bad, dtype)
    with pytest.raises(AssertionError, match=r"worst at row 40,"):
        R.check_pointwise(bad, ref, pre, acc, K, dtype, what="residual shifted")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_block_written_transposed_is_rejected(dtype):
    M, N, K = 64, 64, 320
    A, W, b, _ = _linear(M, N, K, dtype, seed=5)
    ref, pre, acc = _ref(A, W, b, None)
    got = _kernel_like(A, W, b, None, dtype)
    bad = got.clone()
    bad[32:48, 16:32] = got[32:48, 16:32].t()
    with pytest.raises(AssertionError, match=r"worst at row (3[2-9]|4[0-7]), column (1[6-9]|2\d|3[01])"):
        R.check_pointwise(bad, ref, pre, acc, K, dtype, what="transposed block")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_guard_band_sees_a_stray_write_and_a_nan_read(dtype):
    rows, cols, ld, margin = 5, 12, 16, 64
    win, buf = R.out_buffer(rows, cols, ld, margin, dtype, "cpu")
    win.copy_(torch.randn(rows, cols))
    R.check_guard(buf, rows, cols, ld, margin, dtype, what="clean")
    # canonical NaN (what arithmetic writes) differs from the sentinel: a store into the padding columns is seen
    buf.view(-1)[margin + 2 * ld + cols] = math.nan
    with pytest.raises(AssertionError, match=r"row 2, column 12"):
        R.check_guard(buf, rows, cols, ld, margin, dtype, what="stray store")
    win, buf = R.out_buffer(rows, cols, ld, margin, dtype, "cpu")
    win.copy_(torch.randn(rows, cols))
    win[4, 11] = math.nan
    with pytest.raises(AssertionError, match="non-finite"):
        R.check_guard(buf, rows, cols, ld, margin, dtype, what="NaN read")
    # the input side: NaN margins and padding columns, the window intact
    v = torch.randn(3, 5).to(dtype)
    w, b = R.guarded(v, ld=8, margin=10)
    assert torch.equal(w, v) and w.stride() == (8, 1)
    assert torch.isnan(b[:10]).all() and torch.isnan(b[-10:]).all() and torch.isnan(b[10:34].view(3, 8)[:, 5:]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_a_result_that_underflows_passes(dtype):
    """half storage rounds a product of 6e-9 to zero: the bound carries the absolute rounding error of the subnormal range"""
    ref = torch.tensor([[6e-9, -6e-9, 2.0 ** -14]], dtype=torch.float64)
    got = ref.to(dtype)
    z = torch.zeros_like(ref)
    R.check_pointwise(got, ref, z, z, 64, dtype, what="underflow")
    with pytest.raises(AssertionError):
        R.check_pointwise(got + 2 * R.TINY[dtype] + 2.0 ** -22, ref, z, z, 64, dtype, what="underflow, off by more")


def test_sample_rows_cover_tiles_images_and_tail():
    M, img, Wout = 3 * 4096 + 64, 4096, 64
    rows = R.sample_rows(M, n_random=500, image=img, Wout=Wout, cap=4096)
    s = set(rows.tolist())
    assert set(range(256)) <= s and set(range(M // 256 * 256, M)) <= s
    assert set(range(2 * img, 2 * img + Wout)) <= s and set(range(3 * img - Wout, 3 * img)) <= s
    assert rows.numel() <= 4096 + 512 and int(rows.max()) == M - 1
