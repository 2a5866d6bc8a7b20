"""CPU: the references of tests/helpers/precise_ref.py (used by tests/test_gpu_precise_kernels.py) are right, and the product bound
can tell the three-term split-bf16 product from its two cheaper mutants.

The product is emulated the way the kernel computes it (packed operands [hi | hi | lo] x [hi | lo | hi], one fp32-accumulated
contraction over the packed K).  The bound 3 * 2^-16 * mag + accumulation term and the 2^-14 cap on the relative L2 error must accept
it on every element and reject both mutants: `a_lo . w_hi` dropped (a weight-side-only split) and hi parts only (plain bf16)."""
import pytest
import torch

from helpers import precise_ref as R


def _operands(C, M=48, N=40, seed=0):
    """magnitudes spread over 2^-6 .. 2^6"""
    g = torch.Generator().manual_seed(seed + C)
    a = torch.randn(M, C, generator=g) * torch.exp2(torch.rand(M, C, generator=g) * 12 - 6)
    w = torch.randn(N, C, generator=g) * torch.exp2(torch.rand(N, C, generator=g) * 12 - 6)
    return a, w


@pytest.mark.parametrize("C", [3, 64, 100, 512])
def test_product_bound_accepts_three_terms_and_rejects_the_mutants(C):
    a, w = _operands(C)
    Kp = R.split_kp(C)
    ref = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    worst, l2 = R.check_product(R.emulate_product(a, w), ref, mag, Kp, f"emulated C={C}")
    lead = float(((R.emulate_product(a, w).double() - ref).abs() / (3 * 2.0 ** -16 * mag)).max())
    print(f"C={C} Kp={Kp}: three terms worst error/bound {worst:.3f}, error/(3 2^-16 mag) {lead:.3f}, L2 {l2:.2e}")
    assert lead < 1.0
    for variant in ("no_lo_hi", "hi_only"):
        got = R.emulate_product(a, w, variant).double()
        frac = float(((got - ref).abs() > R.product_bound(mag, Kp)).double().mean())
        l2m = float((got - ref).norm() / ref.norm())
        print(f"C={C} {variant}: {100 * frac:.0f} % of the elements out of bound, L2 {l2m:.2e}")
        assert frac > 0.25 and l2m > 8 * R.L2_CAP, (variant, frac, l2m)
        with pytest.raises(AssertionError):
            R.check_product(got, ref, mag, Kp, variant)


def test_geometry_restated():
    # 3C <= 64; 3C % 64 == 0; padded to 64 / 128 / 256
    want = {3: (3, 64), 8: (8, 64), 20: (20, 64), 21: (21, 64), 24: (64, 192), 64: (64, 192), 72: (128, 384), 100: (128, 384),
            128: (128, 384), 200: (256, 768), 512: (512, 1536)}
    for C, (cs, kp) in want.items():
        assert (R.split_cs(C), R.split_kp(C)) == (cs, kp), C
        assert kp % 64 == 0 and 3 * cs <= kp and C <= cs


def _bf16_loop(v):
    """round-to-nearest-even bfloat16 of one Python float held as fp32, by bit arithmetic"""
    import struct
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF
    return u >> 16


def _f32(v):
    import struct
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _from_bits(h):
    import struct
    return struct.unpack("<f", struct.pack("<I", h << 16))[0]


@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("geo", [0, 1, 2])
def test_split3_ref_against_loops(C, geo):
    B, H, W = 2, 4, 2
    g = torch.Generator().manual_seed(C * 10 + geo)
    x = torch.randn(B * H * W, C, generator=g)
    p, q = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    r = R.split3_ref(x, C, R.P_AFFINE, p=p, q=q, pq_img=1, geo=geo, B=B, H=H, W=W)
    Ho, Wo = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[geo]
    assert r["v"].shape == (B * Ho * Wo, C)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                row = (b * Ho + oy) * Wo + ox
                if geo == 2 and (oy % 2 or ox % 2):
                    assert not r["live"][row] and float(r["v"][row].abs().max()) == 0.0
                    continue
                iy, ix = {0: (oy, ox), 1: (2 * oy, 2 * ox), 2: (oy // 2, ox // 2)}[geo]
                src = (b * H + iy) * W + ix
                assert int(r["src"][row]) == src and bool(r["live"][row])
                for c in range(C):
                    want = float(p[b, c]) * float(x[src, c]) + float(q[b, c])
                    assert abs(float(r["v"][row, c]) - want) <= 1e-14 * (1 + abs(want))
    first, mid, last, pad = R.split3_columns(C)
    Cs, Kp = R.split_cs(C), R.split_kp(C)
    assert first.tolist() == list(range(C)) and mid.tolist() == list(range(Cs, Cs + C)) and last.tolist() == list(range(2 * Cs, 2 * Cs + C))
    assert int(pad.sum()) == Kp - 3 * C
    f2, m2, l2, _ = R.split3_columns(C, worder=1)
    assert m2.tolist() == last.tolist() and l2.tolist() == mid.tolist() and f2.tolist() == first.tolist()


def test_ops_match_autograd():
    """the three *_GRAD ops are the derivatives of their forward ops (fp64 autograd), with a z whose signs differ from x's"""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(64, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(64, 7, generator=g, dtype=torch.float64)
    p = torch.randn(1, 7, generator=g, dtype=torch.float64).expand(64, 7)
    q = torch.randn(1, 7, generator=g, dtype=torch.float64).expand(64, 7)
    for fwd, bwd in ((R.P_PRELU, R.P_PRELU_GRAD), (R.P_RELU, R.P_RELU_GRAD), (R.P_QGELU, R.P_QGELU_GRAD)):
        (gz,) = torch.autograd.grad((R.op64(fwd, z, None, p, q) * x).sum(), z)
        assert torch.allclose(gz, R.op64(bwd, x, z.detach(), p, q), rtol=1e-12, atol=1e-14), R.OP_NAMES[bwd]
    t = torch.randn(50, 3, generator=g, dtype=torch.float64)
    assert torch.allclose(R.op64(R.P_GELU, t), torch.nn.functional.gelu(t), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("O,I,k,perm", [(5, 3, 3, (0, 0)), (4, 20, 1, (0, 0)), (3, 20, 1, (4, 5))])
@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_pack_w_ref_against_loops(O, I, k, perm, dgrad, scaled):
    g = torch.Generator().manual_seed(O + I)
    w = torch.randn(O, I, k, k, generator=g)
    scale = torch.randn(O, generator=g) if scaled else None
    perm_hw, perm_c = perm
    NR, NC = (I, O) if dgrad else (O, I)
    rows = (NR + 3) // 4 * 4
    got = R.pack_w_ref(w, scale, O, I, k, dgrad, rows, perm_hw, perm_c)
    Cs, Kp = R.split_cs(NC), R.split_kp(NC)
    kk = k * k
    assert got.shape == (rows, kk, Kp)
    wf = w.reshape(O, I, kk)
    for n in range(rows):
        for tap in range(kk):
            for j in range(Kp):
                part, c = j // Cs, j % Cs
                want = 0
                if part < 3 and c < NC and n < NR:
                    o, i = (c, n) if dgrad else (n, c)
                    t = kk - 1 - tap if dgrad else tap
                    if perm_hw:
                        hw, ch = i // perm_c, i % perm_c
                        i = ch * perm_hw + hw
                    v = float(wf[o, i, t])
                    if scaled:
                        v = _f32(v * float(scale[o]))
                    hi = _bf16_loop(v)
                    want = _bf16_loop(_f32(v - _from_bits(hi))) if part == 1 else hi
                assert (int(got[n, tap, j]) & 0xFFFF) == want, (n, tap, j)
