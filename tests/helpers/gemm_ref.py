"""Pointwise references for the GEMM / 3x3-convolution kernels (csrc/gemm.hip, pgemm.hip, pconv.hip).

* ``rows_operand`` / ``contract``: the fp64 contraction of selected output rows -- the rows of A for a linear layer, an im2col of only
  the sampled output pixels for the three convolution modes (1: zero-padded 3x3, 2: stride 2, 3: on the 2x nearest-upsampled image),
  from the operands as stored (already rounded to the storage format).  Works on whatever device the tensors live on.
* ``check_pointwise``: per element  |got - ref| <= u (|ref| + |pre|) + 2 eta + c sqrt(K) 2^-24 (sum_k |a_k w_k| + |bias| + |res|)
  with u the unit roundoff of the storage format, eta half its smallest subnormal (a result that underflows: half storage rounds
  6e-9 to 0) and pre = the value before the residual add (the epilogue rounds it once on its own: bf16(acc + bias), then + residual,
  rounded again; pre is 0 without a residual).  The sqrt(K) form is what lets one dropped 64-wide
  K-tile (~0.07 per element at K = 11520) stand out of the fp32 accumulation noise; tests/test_host_gemm_ref.py proves that.
* ``guarded`` / ``out_buffer`` / ``check_guard``: every operand sits in the middle of a larger buffer whose margins (and padding columns)
  are NaN, the output inside a buffer prefilled with a NaN bit pattern that arithmetic does not produce, so a read past an operand shows
  up as a non-finite output and a write past the M x N window as a changed sentinel."""
import math

import torch

# unit roundoff of the storage format (round to nearest: half an ulp relative)
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# quiet-NaN bit patterns with a payload: arithmetic only ever produces the canonical 0x7FC0 / 0x7E00 (or their negatives)
SENTINEL = {torch.bfloat16: 0x7FE5, torch.float16: 0x7E5A}
# half the smallest subnormal: the absolute rounding error of a result that underflows
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
C_ACC = 4.0                 # the constant c of the accumulation term
TILE_ROWS = 256


def unit(dtype):
    return UNIT[dtype]


# ---------------------------------------------------------------------------------------------------------- operands of sampled rows
def conv_out_hw(mode, Hin, Win):
    if mode == 1:
        return Hin, Win
    if mode == 2:
        return (Hin + 1) // 2, (Win + 1) // 2
    if mode == 3:
        return 2 * Hin, 2 * Win
    raise ValueError(mode)


def conv_rows(x, rows, mode, Hout, Wout):
    """im2col of the output pixels `rows` (flat NHWC pixel indices over the batch) of a 3x3 convolution, pad 1, on x [B][Hin][Win][Cin]:
    [len(rows)][9 Cin] float64 in the kernels' K order k = (ky * 3 + kx) * Cin + ci; taps outside the (upsampled) image are zero."""
    B, Hin, Win, Cin = x.shape
    rows = rows.to(x.device).long()
    hw = Hout * Wout
    b, r = rows // hw, rows % hw
    oy, ox = r // Wout, r % Wout
    cols = []
    for ky in range(3):
        for kx in range(3):
            if mode == 1:
                iy, ix = oy + ky - 1, ox + kx - 1
                ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            elif mode == 2:
                iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
                ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            else:
                uy, ux = oy + ky - 1, ox + kx - 1
                ok = (uy >= 0) & (uy < 2 * Hin) & (ux >= 0) & (ux < 2 * Win)
                iy, ix = torch.div(uy, 2, rounding_mode="floor"), torch.div(ux, 2, rounding_mode="floor")
            v = x[b, iy.clamp(0, Hin - 1), ix.clamp(0, Win - 1)].double()
            cols.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.cat(cols, dim=1)


def rows_operand(A, rows, mode=0, conv=None):
    """the K-long operand rows of output rows `rows`: A [M][>= K] for a linear layer (mode 0), else conv_rows of A viewed as
    [B][Hin][Win][Cin] with conv = (B, Hin, Win, Cin, Hout, Wout)"""
    if mode == 0:
        return A[rows.to(A.device).long()].double()
    B, Hin, Win, Cin, Hout, Wout = conv
    return conv_rows(A.reshape(B, Hin, Win, Cin), rows, mode, Hout, Wout)


def contract(a_rows, W, block=512):
    """(a W^T, |a| |W|^T) in float64 for a [R][K] and W [N][K], R in blocks (the im2col rows of a K = 11520 layer are large)"""
    Wd = W.double()
    Wa = Wd.abs()
    dots, mags = [], []
    for i in range(0, a_rows.shape[0], block):
        a = a_rows[i:i + block].double()
        dots.append(a @ Wd.t())
        mags.append(a.abs() @ Wa.t())
    return torch.cat(dots), torch.cat(mags)


def reference(dot, mag, bias=None, res_rows=None):
    """(ref, pre, bound terms) of C = dot + bias (+ res): ref and pre in fp64, acc = the magnitude the fp32 accumulation works on"""
    pre = dot.clone()
    acc = mag.clone()
    if bias is not None:
        b = bias.double().to(dot.device)[None, :]
        pre = pre + b
        acc = acc + b.abs()
    if res_rows is None:
        return pre, torch.zeros_like(pre), acc
    r = res_rows.double().to(dot.device)
    return pre + r, pre, acc + r.abs()


def bound(ref, pre, acc, K, dtype, c=C_ACC):
    return unit(dtype) * (ref.abs() + pre.abs()) + 2 * TINY[dtype] + c * math.sqrt(K) * 2.0 ** -24 * acc


# ---------------------------------------------------------------------------------------------------------- comparator
def check_pointwise(got, ref, pre, acc, K, dtype, rows=None, tile=(TILE_ROWS, None), what="", c=C_ACC, lim=None):
    """assert |got - ref| <= bound elementwise (got [R][N] in any float format, ref / pre / acc from `reference`); `lim`, if given,
    replaces the bound.  On failure the message names the worst element (ratio error / bound) with its row, column and (row, column)
    tile.  Returns the worst ratio (the margin: < 1 passes)."""
    g = got.double().to(ref.device)
    err = (g - ref).abs()
    b = bound(ref, pre, acc, K, dtype, c) if lim is None else lim
    ratio = torch.where(torch.isfinite(g), err / b.clamp_min(1e-300), torch.full_like(err, math.inf))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = int(ratio.argmax())
        r, col = divmod(i, ratio.shape[1])
        row = int(rows[r]) if rows is not None else r
        tm, tn = tile
        tloc = f"tile ({row // tm}, {col // tn})" if tn else f"row tile {row // tm}"
        bad = int((ratio > 1).sum())
        raise AssertionError(f"{what}: {bad} elements out of bound; worst at row {row}, column {col} ({tloc}): got {float(g.view(-1)[i]):.6g}, "
                             f"want {float(ref.view(-1)[i]):.6g}, |err| {float(err.view(-1)[i]):.3g} > bound {float(b.view(-1)[i]):.3g} "
                             f"(x{worst:.3g})")
    return worst


def sample_rows(M, n_random=1024, image=0, Wout=0, cap=4096, seed=0):
    """output rows to check: the first and the last 256-row tile (with the ragged tail), for a convolution also the first and the last
    image row of the first and of the last image, and a random sample -- sorted, unique, at most `cap`"""
    parts = [torch.arange(0, min(M, TILE_ROWS)), torch.arange(max(0, (M - 1) // TILE_ROWS * TILE_ROWS), M)]
    if image:
        last = (M // image - 1) * image
        for base in (0, last):
            parts += [torch.arange(base, base + Wout), torch.arange(base + image - Wout, base + image)]
    g = torch.Generator().manual_seed(seed)
    parts.append(torch.randint(0, M, (n_random,), generator=g))
    rows = torch.unique(torch.cat(parts).clamp(0, M - 1))
    if rows.numel() > cap:
        keep = torch.randperm(rows.numel(), generator=g)[:cap]
        rows = torch.unique(torch.cat([rows[:TILE_ROWS], rows[keep], rows[-TILE_ROWS:]]))
    return rows


# ---------------------------------------------------------------------------------------------------------- guard bands
def guarded(values, ld=None, margin=0):
    """a copy of `values` ([rows][cols], or 1-D) inside a NaN-filled buffer: `margin` elements on either side and, with ld > cols,
    NaN padding columns.  Returns (window view [rows][cols] with row stride ld, the buffer)."""
    if values.dim() == 1:
        buf = torch.full((2 * margin + values.numel(),), math.nan, dtype=values.dtype, device=values.device)
        win = buf[margin:margin + values.numel()]
        win.copy_(values)
        return win, buf
    rows, cols = values.shape
    ld = cols if ld is None else ld
    buf = torch.full((2 * margin + rows * ld,), math.nan, dtype=values.dtype, device=values.device)
    win = buf[margin:margin + rows * ld].view(rows, ld)[:, :cols]
    win.copy_(values)
    return win, buf


def out_buffer(rows, cols, ld, margin, dtype, device):
    """the output window [rows][cols] at row stride ld inside a buffer of SENTINEL bits, `margin` elements either side"""
    buf = torch.full((2 * margin + rows * ld,), SENTINEL[dtype], dtype=torch.int16, device=device).view(dtype)
    return buf[margin:margin + rows * ld].view(rows, ld)[:, :cols], buf


def check_guard(buf, rows, cols, ld, margin, dtype, what=""):
    """every element outside the window is still the sentinel, the window is finite"""
    bits = buf.view(torch.int16).clone()
    win_bits = bits[margin:margin + rows * ld].view(rows, ld)[:, :cols]
    win = win_bits.view(dtype)
    nonfinite = int((~torch.isfinite(win)).sum())
    assert nonfinite == 0, f"{what}: {nonfinite} non-finite elements inside the output window (an operand read past its extent?)"
    win_bits.fill_(SENTINEL[dtype])
    changed = torch.nonzero(bits != SENTINEL[dtype]).flatten()
    if changed.numel():
        i = int(changed[0]) - margin
        where = f"element {i} before the window" if i < 0 else f"row {i // ld}, column {i % ld} (ld {ld})"
        raise AssertionError(f"{what}: {changed.numel()} elements written outside the {rows} x {cols} window; first at {where}")
