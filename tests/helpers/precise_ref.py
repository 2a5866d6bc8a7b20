"""References for the kernels of the "precise" (split-bf16) path: csrc/pnet.hip, encoder.hip and the gradient kernels of vit.hip
(tests/test_gpu_precise_kernels.py; proved on the CPU by tests/test_host_precise_ref.py).  CPU, torch fp64.

* ``split_cs`` / ``split_kp``: the operand geometry of csrc/pnet.h restated.
* ``op64`` + ``op_allowance``: the ten element-wise ops of the split3 pass in fp64 and what fp32 arithmetic may differ by.
* ``geo_rows`` / ``split3_ref``: the row geometry (0 plain, 1 every second pixel of every second row, 2 zero-stuffed) and the
  column layout [0, C) hi, [Cs, Cs + C) hi, [2 Cs, 2 Cs + C) lo (worder: hi, lo, hi), everything else zero.
* ``pack_w_ref``: the packed weight, bit for bit (one fp32 multiply and two bfloat16 roundings are its only arithmetic).
* ``product_bound``: |got - ref| <= 3 * 2^-16 * mag + c sqrt(K) 2^-24 acc, mag = |a| |w|^T in fp64.  bfloat16's unit roundoff is 2^-8,
  so |lo| <= 2^-8 |v| and hi + lo is off by at most 2^-16 |v| per operand (two terms); the dropped lo * lo product is at most
  2^-16 |a| |w| (the third).  The second summand is gemm_ref.bound's accumulation term at the PACKED K, on the magnitude the fp32
  accumulator really sums: |hi| <= (1 + 2^-8) |v| and |lo| <= 2^-8 |v| make the three partial products at most (1 + 2^-6) mag.
  ``L2_CAP`` = 2^-14 bounds the relative L2 error of a whole output: a quarter of what one missing cross term leaves (2^-8 / sqrt 3
  relative per operand element, ~1.6e-3 measured) would already be 25 times it.
* ``Margins``: the worst error / bound ratio per kernel, written as a table when HEDIT_MARGINS_REPORT names a file.
* fp32 kernels that are not bit-exact get |got - ref| <= (n + 2) 2^-24 S with S the sum of the absolute values of the terms and n the
  longest dependent chain; ``EXP_REL(x)`` = (|x| + 4) 2^-23 is added per fast exponential (argument scaling |x| 2^-24, the hardware
  exp2 and the two roundings around it)."""
import math
import os

import torch

U32 = 2.0 ** -24
L2_CAP = 2.0 ** -14
C_ACC = 4.0          # gemm_ref.C_ACC
P_COPY, P_AFFINE, P_PRELU, P_PRELU_GRAD, P_RELU, P_RELU_GRAD, P_QGELU, P_QGELU_GRAD, P_AFFINE_RELU, P_GELU = range(10)
OP_NAMES = ["copy", "affine", "prelu", "prelu_grad", "relu", "relu_grad", "qgelu", "qgelu_grad", "affine_relu", "gelu"]
GRAD_OPS = (P_PRELU_GRAD, P_RELU_GRAD, P_QGELU_GRAD)
AFFINE_OPS = (P_AFFINE, P_AFFINE_RELU)
SENT32 = 0x7FE5A5A5      # a quiet NaN with a payload: arithmetic produces 0x7FC00000 only


def split_cs(C):
    return C if (3 * C) % 64 == 0 or 3 * C <= 64 else (C + 63) // 64 * 64


def split_kp(C):
    return (3 * split_cs(C) + 63) // 64 * 64


def EXP_REL(x):
    return (x.abs() + 4.0) * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- split3
def hi_lo(v32):
    """(hi, lo) as float32 values of a float32 tensor: hi = bf16(v), lo = bf16(v - hi) -- v - hi is exact in fp32"""
    hi = v32.to(torch.bfloat16).float()
    lo = (v32 - hi).to(torch.bfloat16).float()
    return hi, lo


def op64(op, x, z=None, p=None, q=None):
    """the op on float64 tensors broadcast to x's shape (p, q already expanded to it, or None)"""
    zero = torch.zeros_like(x)
    qq = zero if q is None else q
    if op == P_COPY:
        return x
    if op == P_AFFINE:
        return p * x + q
    if op == P_AFFINE_RELU:
        return (p * x + q).clamp_min(0)
    if op == P_PRELU:
        t = x + qq
        return torch.where(t > 0, t, p * t)
    if op == P_PRELU_GRAD:
        return x * torch.where(z + qq > 0, torch.ones_like(x), p)
    if op == P_RELU:
        return (x + qq).clamp_min(0)
    if op == P_RELU_GRAD:
        return torch.where(z + qq > 0, x, zero)
    if op == P_QGELU:
        t = x + qq
        return t * torch.sigmoid(1.702 * t)
    if op == P_QGELU_GRAD:
        t = z + qq
        s = torch.sigmoid(1.702 * t)
        return x * (s * (1 + 1.702 * t * (1 - s)))
    if op == P_GELU:
        t = x + qq
        return 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))
    raise ValueError(op)


def op_allowance(op, x, z=None, p=None, q=None):
    """|fp32 op - fp64 op| <= this.  (n + 2) u S with the terms' magnitudes S; a step function of t (the sign tests) is exact unless t
    itself rounds across 0, which the test data keep away from (|t| >= 2^-10 there)."""
    ax = x.abs()
    aq = torch.zeros_like(x) if q is None else q.abs()
    if op == P_COPY:
        return torch.zeros_like(x)
    if op in AFFINE_OPS:            # one product, one sum
        return 4 * U32 * (p.abs() * ax + aq)
    if op in (P_PRELU, P_RELU):     # one sum, one product
        return 4 * U32 * (ax + aq) * (1 if p is None else p.abs().clamp_min(1.0))
    if op in (P_PRELU_GRAD, P_RELU_GRAD):
        return 3 * U32 * ax * (1 if p is None else p.abs().clamp_min(1.0))
    if op == P_QGELU:               # t / (1 + e): sum, scale, exp, sum, quotient; d sigmoid = s (1 - s) d(arg) <= EXP_REL / 4
        t = x.abs() + aq
        return t * (6 * U32 + EXP_REL(1.702 * t))
    if op == P_QGELU_GRAD:          # x * (s * (1 + 1.702 t (1 - s))): |1.702 t (1 - s)| and s in [0, 1]-ish factors, eight roundings
        t = z.abs() + aq
        return ax * (1 + 1.702 * t) * (10 * U32 + 2 * EXP_REL(1.702 * t))
    if op == P_GELU:                # erff is accurate to a few ulp (<= 4) of a value in [-1, 1]
        t = x.abs() + aq
        return t * 10 * U32
    raise ValueError(op)


def geo_rows(geo, B, H, W):
    """(input row of every output row, live mask) of a [B][H][W] pixel grid: geo 0 identity; 1 pixel (2 oy, 2 ox); 2 zero-stuffed 2H x 2W"""
    if geo == 0:
        r = torch.arange(B * H * W)
        return r, torch.ones_like(r, dtype=torch.bool)
    Ho, Wo = (H // 2, W // 2) if geo == 1 else (2 * H, 2 * W)
    r = torch.arange(B * Ho * Wo)
    b, rr = r // (Ho * Wo), r % (Ho * Wo)
    oy, ox = rr // Wo, rr % Wo
    if geo == 1:
        return (b * H + 2 * oy) * W + 2 * ox, torch.ones_like(r, dtype=torch.bool)
    return (b * H + oy // 2) * W + ox // 2, (oy % 2 == 0) & (ox % 2 == 0)


def expand_pq(t, pq_img, B, rows_per_img, C):
    """p / q as [rows_in][C] float64"""
    if t is None:
        return None
    t = t.double()
    if pq_img:
        return t.reshape(B, 1, C).expand(B, rows_per_img, C).reshape(B * rows_per_img, C)
    return t.reshape(1, C).expand(B * rows_per_img, C)


def split3_ref(x, C, op, z=None, p=None, q=None, pq_img=0, geo=0, B=1, H=1, W=1):
    """x [rows_in][C] (fp32 values) -> dict: v [rows_out][C] fp64 the op's value (0 in dead rows), allow (same shape), live [rows_out],
    src [rows_out] input rows.  Without geo / pq_img: rows_in = x.shape[0], B = 1."""
    rows_in = x.shape[0]
    if geo == 0 and not pq_img:
        B, H, W = 1, rows_in, 1
    per = H * W
    x64 = x.double()
    z64 = None if z is None else z.double()
    pe, qe = expand_pq(p, pq_img, B, per, C), expand_pq(q, pq_img, B, per, C)
    v = op64(op, x64, z64, pe, qe)
    al = op_allowance(op, x64, z64, pe, qe)
    src, live = geo_rows(geo, B, H, W)
    v, al = v[src], al[src]
    v[~live] = 0
    al[~live] = 0
    return {"v": v, "allow": al, "live": live, "src": src}


def split3_columns(C, worder=0):
    """(hi columns, second hi columns, lo columns, pad mask [Kp]) of the operand row"""
    Cs, Kp = split_cs(C), split_kp(C)
    c = torch.arange(C)
    first, mid, last = c, Cs + c, 2 * Cs + c
    pad = torch.ones(Kp, dtype=torch.bool)
    pad[first] = pad[mid] = pad[last] = False
    return (first, last, mid, pad) if worder else (first, mid, last, pad)


# ---------------------------------------------------------------------------------------------------------------- weights
def pack_w_ref(w, scale, O, I, k, dgrad, rows_out, perm_hw=0, perm_c=0):
    """w fp32 [O][I][k][k] -> int16 bits [rows_out][k k][Kp] of the bf16 operand, parts (hi, lo, hi)"""
    kk = k * k
    ws = w.float().reshape(O, I, kk)
    if scale is not None:
        ws = ws * scale.float().reshape(O, 1, 1)            # one fp32 multiply
    if perm_hw > 0:      # packed input index (hw, ch) <- torch's (ch, hw)
        ws = ws.reshape(O, perm_c, perm_hw, kk).permute(0, 2, 1, 3).reshape(O, I, kk)
    if dgrad:
        m = ws.flip(2).permute(1, 2, 0)                     # [I][tap flipped][O]
        NR, NC = I, O
    else:
        m = ws.permute(0, 2, 1)                             # [O][tap][I]
        NR, NC = O, I
    Cs, Kp = split_cs(NC), split_kp(NC)
    hi, lo = hi_lo(m.contiguous())
    out = torch.zeros(rows_out, kk, Kp, dtype=torch.bfloat16)
    out[:NR, :, 0:NC] = hi.to(torch.bfloat16)
    out[:NR, :, Cs:Cs + NC] = lo.to(torch.bfloat16)
    out[:NR, :, 2 * Cs:2 * Cs + NC] = hi.to(torch.bfloat16)
    return out.view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- product
def product_bound(mag, K_packed):
    return 3 * 2.0 ** -16 * mag + C_ACC * math.sqrt(K_packed) * U32 * (1 + 2.0 ** -6) * mag


def check_product(got, ref, mag, K_packed, what, margins=None):
    """the pointwise bound on every element and the L2 cap; returns (worst ratio, relative L2)"""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    ratio = ((g - ref).abs() / product_bound(mag, K_packed).clamp_min(1e-300))
    worst = float(ratio.max())
    l2 = float((g - ref).norm() / ref.norm().clamp_min(1e-300))
    if margins is not None:
        margins.add(what, worst, f"L2 {l2:.2e}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound, worst x{worst:.3g}"
    assert l2 < L2_CAP, f"{what}: relative L2 error {l2:.3e} >= 2^-14"
    return worst, l2


def emulate_product(a, w, variant="full"):
    """the kernel's arithmetic on the CPU: packed operands, ONE fp32-accumulated contraction.  a [M][C], w [N][C] fp32.
    variant: full | no_lo_hi (a_lo . w_hi dropped) | hi_only"""
    C = a.shape[1]
    Cs, Kp = split_cs(C), split_kp(C)
    ah, al = hi_lo(a.float())
    wh, wl = hi_lo(w.float())
    A = torch.zeros(a.shape[0], Kp)
    Wp = torch.zeros(w.shape[0], Kp)
    A[:, 0:C], A[:, Cs:Cs + C], A[:, 2 * Cs:2 * Cs + C] = ah, ah, al
    Wp[:, 0:C], Wp[:, Cs:Cs + C], Wp[:, 2 * Cs:2 * Cs + C] = wh, wl, wh
    if variant in ("no_lo_hi", "hi_only"):
        A[:, 2 * Cs:2 * Cs + C] = 0
    if variant == "hi_only":
        Wp[:, Cs:Cs + C] = 0
    return A @ Wp.t()


# ---------------------------------------------------------------------------------------------------------------- fp32 kernels
def check_bound(got, ref, bound, what, margins=None):
    g = got.double().cpu()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if margins is not None:
        margins.add(what, worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound; worst at flat index {i}: got "
                             f"{float(g.reshape(-1)[i]):.9g}, want {float(ref.reshape(-1)[i]):.9g}, bound {float(bound.reshape(-1)[i]):.3g} (x{worst:.3g})")
    return worst


class Margins:
    """worst error / bound per kernel; appended to $HEDIT_MARGINS_REPORT as `storage kernel worst note`"""

    def __init__(self):
        self.rows = {}

    def add(self, what, worst, note=""):
        key = what.split(" ")[0]
        if key not in self.rows or worst > self.rows[key][0]:
            self.rows[key] = (worst, note)
        print(f"margin {what}: error / bound = {worst:.3g} {note}")
        rep = os.environ.get("HEDIT_MARGINS_REPORT")
        if rep:
            with open(rep, "a") as f:
                f.write(f"{os.environ.get('HEDIT_STORAGE', 'bf16')}\t{what}\t{worst:.3e}\t{note}\n")


def out32(n, device, margin=64):
    """(window [n] fp32, whole buffer) prefilled with SENT32 bits"""
    buf = torch.full((n + 2 * margin,), SENT32, dtype=torch.int32, device=device).view(torch.float32)
    return buf[margin:margin + n], buf


def check_guard32(buf, n, what, margin=64, finite=True):
    bits = buf.view(torch.int32)
    assert bool((bits[:margin] == SENT32).all()) and bool((bits[margin + n:] == SENT32).all()), f"{what}: written outside its output"
    win = bits[margin:margin + n]
    assert not bool((win == SENT32).any()), f"{what}: output elements left unwritten"
    if finite:
        assert bool(torch.isfinite(buf[margin:margin + n]).all()), f"{what}: non-finite output (an input read past its extent?)"


def nan_guarded(t, device, margin=64):
    """a device copy of the fp32 tensor t between NaN margins"""
    flat = t.reshape(-1).float()
    buf = torch.full((flat.numel() + 2 * margin,), math.nan, dtype=torch.float32, device=device)
    win = buf[margin:margin + flat.numel()]
    win.copy_(flat)
    return win.view(t.shape)
