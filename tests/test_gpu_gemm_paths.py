"""-m gpu: every dispatch path of gemm_launch (csrc/gemm.hip) against an fp64 reference, pointwise, with guard bands.

gemm_launch picks one of about a dozen kernels for a linear layer or a 3x3 convolution by shape, split count and CU count: the
persistent pgemm / pconv (>= 2 x CUs tiles of 256 rows), igemm_kernel's 256-row one-shot tile (plain, chunk fold, row-sharing modes 4 / 5),
its 128-row tile with the two-stage loop or the three-stage DEEP ring, split-K slabs with splitk_reduce / splitk_reduce_gn, and the
GEGLU tiles.  Each case below names the path it must reach; `path` restates the selection rules of launch_igemm, gemm_launch,
pgemm_supported and pconv_supported, so a shape that drifts off its path fails instead of quietly testing another one.

Every case asserts
  1. the pointwise fp64 bound of tests/helpers/gemm_ref.py on sampled rows (first / last tile, first / last image rows, a random sample);
  2. intact guard bands: NaN around every operand (and in its padding columns), a sentinel around the output window;
  3. identical bits from a second launch;
  4. persistent paths: identical bits from the one-shot kernel (test flag 8);
  5. where a launch of the first tile / image alone takes another path: identical bits for those rows (batch invariance across the
     path boundary).
The M-sweep at the UNet's (N, K) pairs launches one operand set at row counts on either side of every threshold, with the split count
unet.hip::run_gemm would choose, and asserts that every launch's rows equal the largest launch's."""
import math

import pytest
import torch

from helpers import gemm_ref as R
from hedit import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BK = 64


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.lib()


@pytest.fixture(scope="module")
def cus(lib):
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------- the selection rules
def pick_bn(N):
    return 160 if cdiv(N, 160) * 160 <= cdiv(N, 128) * 128 else 128


def resolve_splits(K, splits):
    """hedit_k_gemm / gemm_launch: (split-K slabs, chunk length in K-tiles of the in-register fold) of a `splits` argument"""
    kt = K // BK
    pick = (lambda f: 1 if f <= 1 else min(f, kt))
    if splits < 0:
        slabs, chunk = 1, cdiv(kt, pick(-splits))
    else:
        slabs, chunk = pick(splits), 0
    if chunk >= kt:
        chunk = 0
    if slabs > 1:
        slabs = cdiv(kt, cdiv(kt, slabs))
    return slabs, chunk


def path(cus, M, N, K, mode=0, hw=(0, 0, 0, 0), splits=0, res=False, lda=None, ldc=None, ldr=None, geglu=False, gn=False, flags=0):
    """(kernel, column tile, chunk fold, split-K slabs) gemm_launch runs for this launch -- pgemm_supported, pconv_supported and
    launch_igemm restated.  kernel: pgemm | pconv | rowshare (igemm modes 4 / 5) | igemm256 | igemm128deep | igemm128 | geglu256"""
    Hin, Win, Hout, Wout = hw
    kt = K // BK
    lda, ldc, ldr = lda or K, ldc or N, ldr or N
    slabs, chunk = (1, 0) if geglu else resolve_splits(K, splits)
    if geglu:
        bn = 256 if N % 256 == 0 and cdiv(M, 256) * (N // 256) >= 200 else 128
    else:
        bn = pick_bn(N)
    if slabs == 1 and chunk and mode == 3:
        bn = 128
    same = Hout == Hin and Wout == Win and Win > 0 and 256 % Win == 0
    if slabs == 1 and chunk and mode == 1 and same and N % 128 == 0 and cdiv(M, 256) * (N // 128) >= 512:
        bn = 128
    t256 = cdiv(M, 256) * cdiv(N, bn)
    rows16 = N % 8 == 0 and ldc % 8 == 0 and (not res or ldr % 8 == 0)
    if not flags & 8 and slabs == 1 and not geglu and not gn:
        if mode == 0 and not chunk and bn in (128, 160) and kt >= 3 and rows16 and lda % 8 == 0 and t256 >= 2 * cus:
            return "pgemm", bn, False, 1
        up_ok = Wout > 0 and 256 % Wout == 0 and Hout == 2 * Hin and Wout == 2 * Win
        if ((mode == 1 and same) or (mode == 3 and up_ok)) and (bn == 128 or (bn == 160 and not chunk)) and kt >= 16 and rows16 \
                and N % bn == 0 and not (mode == 3 and (chunk or Wout > 128)) and t256 >= 2 * cus:
            return "pconv", bn, bool(chunk), 1
    if bn == 256:
        return "geglu256", 256, False, 1
    big = slabs == 1 and (geglu or kt >= 16) and t256 >= 200
    fold = slabs == 1 and chunk > 0
    if big and ((mode == 1 and same) or (mode == 3 and Wout > 0 and 256 % Wout == 0)):
        if not fold:
            return "rowshare", bn, False, 1
        if bn == 128:
            return "rowshare", bn, True, 1
    if fold:
        return ("igemm256" if big else "igemm128"), bn, True, 1
    if big:
        return "igemm256", bn, False, 1
    if cdiv(M, 128) * cdiv(N, bn) * slabs <= cus and kt >= 3:
        return "igemm128deep", bn, False, slabs
    return "igemm128", bn, False, slabs


# ---------------------------------------------------------------------------------------------------------- the cases
# spec(cus) -> dict: mode, N, K (linear) or Cin + (B, Hin) (conv, square images), splits, res / bias, padded strides,
# kind (gemm | conv_gn | geglu), and `want` = the path it must reach.  Persistent cases are sized from the CU count.
def _lin(M, N, K, want, **kw):
    return dict(kind="gemm", mode=0, M=M, N=N, K=K, want=want, **kw)


def _conv(mode, B, Hin, Cin, N, want, **kw):
    Hout = Hin if mode == 1 else (Hin // 2 if mode == 2 else 2 * Hin)
    return dict(kind=kw.pop("kind", "gemm"), mode=mode, B=B, Hin=Hin, Hout=Hout, Cin=Cin, M=B * Hout * Hout, N=N, K=9 * Cin, want=want, **kw)


CASES = {
    # persistent linear: both column tiles, residual on / off, ragged M, ragged N, K = 3 tiles, padded lda / ldc / ldr
    "pgemm-160-res-ragged-M-ldc": lambda c: _lin(256 * cdiv(2 * c, 4) + 72, 640, 640, ("pgemm", 160, False, 1), res=True, ldc=960),
    "pgemm-160-nores-ragged-N-lda": lambda c: _lin(256 * cdiv(2 * c, 4) + 8, 600, 320, ("pgemm", 160, False, 1), lda=384),
    "pgemm-128-res-N200-K192-ldr": lambda c: _lin(256 * cdiv(2 * c, 2) + 100, 200, 192, ("pgemm", 128, False, 1), res=True, ldr=256),
    "pgemm-128-nores-K192-lda-ldc": lambda c: _lin(256 * cdiv(2 * c, 8), 1024, 192, ("pgemm", 128, False, 1), lda=256, ldc=1152),
    # persistent row-sharing 3x3: both column tiles, chunk fold, W = 8 with a ragged tail, upsampling gather, the concat write
    "pconv-160-res-concat": lambda c: _conv(1, cdiv(2 * c, 8), 32, 128, 320, ("pconv", 160, False, 1), res=True, ldc=640),
    "pconv-128-nores-W8-ragged": lambda c: _conv(1, 4 * c + 1, 8, 128, 256, ("pconv", 128, False, 1)),
    "pconv-128-fold-res": lambda c: _conv(1, c, 16, 128, 256, ("pconv", 128, True, 1), res=True, splits=-2),
    "pconv-up-160-res-concat": lambda c: _conv(3, cdiv(2 * c, 8), 16, 128, 320, ("pconv", 160, False, 1), res=True, ldc=480),
    "pconv-up-128-nores": lambda c: _conv(3, 2 * c, 8, 128, 128, ("pconv", 128, False, 1)),
    # the 256-row one-shot tile (200 <= tiles < 2 x CUs): linear, conv modes 1 / 2 / 3 off the row-sharing loop, modes 4 / 5
    "igemm256-linear-res": lambda c: _lin(256 * 60, 640, 1024, ("igemm256", 160, False, 1), res=True),
    "igemm256-linear-fold": lambda c: _lin(256 * 60 + 40, 640, 1024, ("igemm256", 160, True, 1), res=True, splits=-4),
    "igemm256-conv-W24": lambda c: _conv(1, 49, 24, 128, 320, ("igemm256", 160, False, 1), res=True),
    "igemm256-conv-stride2": lambda c: _conv(2, 30, 64, 128, 320, ("igemm256", 160, False, 1)),
    "igemm256-conv-up-W24": lambda c: _conv(3, 49, 12, 128, 320, ("igemm256", 160, False, 1), res=True),
    "rowshare-160-res": lambda c: _conv(1, 30, 32, 128, 320, ("rowshare", 160, False, 1), res=True),
    "rowshare-128-fold": lambda c: _conv(1, 30, 32, 128, 256, ("rowshare", 128, True, 1), splits=-2),
    "rowshare-up-160": lambda c: _conv(3, 30, 16, 128, 320, ("rowshare", 160, False, 1), res=True),
    # the 128-row tile: DEEP at blocks = CUs, two-stage one row past it, below DEEP's three K-tiles
    "igemm128deep-at-cus-K192": lambda c: _lin(128 * (c // 4), 640, 192, ("igemm128deep", 160, False, 1), res=True),
    "igemm128-past-cus-K192": lambda c: _lin(128 * (c // 4) + 1, 640, 192, ("igemm128", 160, False, 1), res=True),
    "igemm128-K64": lambda c: _lin(1000, 640, 64, ("igemm128", 160, False, 1), res=True),
    "igemm128-K128": lambda c: _lin(5000, 320, 128, ("igemm128", 160, False, 1)),
    "igemm128deep-conv": lambda c: _conv(1, 2, 16, 128, 320, ("igemm128deep", 160, False, 1), res=True),
    # split-K slabs + splitk_reduce (with / without bias and residual), + splitk_reduce_gn
    "splitk-bias-res": lambda c: _lin(512, 1280, 2560, ("igemm128deep", 160, False, 4), res=True, splits=4),
    "splitk-plain": lambda c: _lin(512 + 36, 1280, 2560, ("igemm128deep", 160, False, 4), bias=False, splits=4),
    "splitk-conv-up": lambda c: _conv(3, 2, 8, 128, 640, ("igemm128deep", 160, False, 3), res=True, splits=3),
    "splitk-gn-conv": lambda c: _conv(1, 2, 16, 128, 256, ("igemm128deep", 128, False, 2), res=True, splits=2, kind="conv_gn"),
    # GEGLU: the 256-column tile, the 128-column tile on the 256-row and on the 128-row kernel
    "geglu-256": lambda c: dict(kind="geglu", mode=0, M=256 * 20, N=2560, K=320, ldc=1408, want=("geglu256", 256, False, 1)),
    "geglu-128-big": lambda c: dict(kind="geglu", mode=0, M=256 * 100, N=320, K=320, want=("igemm256", 128, False, 1)),
    "geglu-128": lambda c: dict(kind="geglu", mode=0, M=1000, N=320, K=64, ldc=168, want=("igemm128", 128, False, 1)),
}


# ---------------------------------------------------------------------------------------------------------- operands and launches
class Problem:
    """one case's operands, each inside a NaN guard band (tests/helpers/gemm_ref.py)"""

    def __init__(self, lib, spec, seed):
        self.lib, self.s = lib, spec
        self.dt = _lib.storage_dtype()
        s = spec
        self.mode, self.M, self.N, self.K = s["mode"], s["M"], s["N"], s["K"]
        self.kind = s["kind"]
        self.splits = s.get("splits", 0)
        self.lda = s.get("lda", self.K) if self.mode == 0 else s["Cin"]
        self.ldc = s.get("ldc", self.N // 2 if self.kind == "geglu" else self.N)
        self.ldr = s.get("ldr", self.N)
        self.n_out = self.N // 2 if self.kind == "geglu" else self.N
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = (lambda *shape, sc=1.0: torch.randn(*shape, generator=g, device=DEV) * sc)      # noqa: E731
        if self.mode == 0:
            self.conv, self.hw = None, (0, 0, 0, 0)
            self.A, self._ab = R.guarded(rn(self.M, self.K).to(self.dt), ld=self.lda, margin=256 * self.lda)
        else:
            B, Hin, Hout, Cin = s["B"], s["Hin"], s["Hout"], s["Cin"]
            self.conv = (B, Hin, Hin, Cin, Hout, Hout)
            self.hw = (Hin, Hin, Hout, Hout)
            self.A, self._ab = R.guarded(rn(B * Hin * Hin, Cin).to(self.dt), margin=(256 + Hin) * Cin)
        self.W, self._wb = R.guarded(rn(self.N, self.K, sc=self.K ** -0.5).to(self.dt), margin=256 * self.K)
        self.bias = R.guarded(rn(self.N), margin=256)[0] if s.get("bias", True) else None
        self.res = R.guarded(rn(self.M, self.N).to(self.dt), ld=self.ldr, margin=256 * self.ldr)[0] if s.get("res") else None
        self.gn = None

    def path(self, cus, M=None, flags=0, splits=None):
        return path(cus, self.M if M is None else M, self.N, self.K, self.mode, self.hw, self.splits if splits is None else splits,
                    self.res is not None, self.lda, self.ldc, self.ldr, geglu=self.kind == "geglu", gn=self.kind == "conv_gn", flags=flags)

    def launch(self, M=None, splits=None):
        """-> (output window, its sentinel buffer, margin); M < self.M = the first M rows (conv: whole images) alone"""
        M = self.M if M is None else M
        splits = self.splits if splits is None else splits
        margin = 256 * self.ldc
        out, buf = R.out_buffer(M, self.n_out, self.ldc, margin, self.dt, DEV)
        p, lib = _lib.ptr, self.lib
        conv5 = self.hw[:2] + (self.lda,) + self.hw[2:] if self.mode else (0, 0, 0, 0, 0)
        ws = torch.empty(max(lib.hedit_k_gemm_ws_bytes(M, self.N, self.K, splits), 16), dtype=torch.uint8, device=DEV)
        if self.kind == "geglu":
            _lib.check(lib.hedit_k_gemm_geglu(p(self.A), p(self.W), p(self.bias), p(out), M, self.N // 2, self.K, self.lda, self.ldc, None))
        elif self.kind == "conv_gn":
            self.gn = torch.full((M // 128, self.N // 2, 2), math.nan, dtype=torch.float32, device=DEV)
            _lib.check(lib.hedit_k_conv_gn(p(self.A), p(self.W), p(self.bias), p(self.res), p(out), M, self.N, self.K, self.ldc, self.ldr,
                                           self.mode, *conv5, splits, p(ws), p(self.gn), None))
        else:
            _lib.check(lib.hedit_k_gemm(p(self.A), p(self.W), p(self.bias), p(self.res), p(out), M, self.N, self.K, self.lda, self.ldc,
                                        self.ldr, self.mode, *conv5, splits, p(ws), None))
        torch.cuda.synchronize()
        return out, buf, margin

    def check(self, out, what):
        """the pointwise fp64 bound on sampled rows -> worst margin"""
        img = self.conv[4] * self.conv[5] if self.conv else 0
        rows = R.sample_rows(self.M, n_random=1024, image=img, Wout=self.conv[5] if self.conv else 0, seed=self.M).to(DEV)
        a = R.rows_operand(self.A, rows, self.mode, self.conv)
        got = out[rows]
        if self.kind != "geglu":
            dot, mag = R.contract(a, self.W)
            ref, pre, acc = R.reference(dot, mag, self.bias, None if self.res is None else self.res[rows])
            return R.check_pointwise(got, ref, pre, acc, self.K, self.dt, rows=rows, tile=(256, self.s["want"][1]), what=what)
        # GEGLU: packed weight rows (value 16 | gate 16) -> output column c = value row t*32 + u, gate row t*32 + 16 + u (c = 16 t + u)
        c = torch.arange(self.n_out, device=DEV)
        rv = (c // 16) * 32 + c % 16
        dot, mag = R.contract(a, self.W)
        b = self.bias.double()
        v, gt = dot[:, rv] + b[rv], dot[:, rv + 16] + b[rv + 16]
        sv, sg = mag[:, rv] + b[rv].abs(), mag[:, rv + 16] + b[rv + 16].abs()
        gelu = 0.5 * gt * (1.0 + torch.erf(gt / math.sqrt(2.0)))
        ref = v * gelu
        # accumulation error of v and g carried through the product (|gelu'| < 1.13), the polynomial erf (~3e-7), the output rounding
        lim = R.unit(self.dt) * ref.abs() + R.TINY[self.dt] + R.C_ACC * math.sqrt(self.K) * 2.0 ** -24 * (sv * gelu.abs() + 1.13 * v.abs() * sg) \
            + 1e-6 * v.abs() * (gt.abs() + 1.0)
        return R.check_pointwise(got, ref, None, None, self.K, self.dt, rows=rows, tile=(256, 128), what=what, lim=lim)


def _small_rows(pb):
    """the first tile (linear) or the first image (conv) launched alone"""
    return pb.conv[4] * pb.conv[5] if pb.conv else 256


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_path_matches_fp64(lib, cus, name):
    spec = CASES[name](cus)
    pb = Problem(lib, spec, seed=sum(map(ord, name)))
    got_path = pb.path(cus)
    assert got_path == spec["want"], f"{name}: the shape reaches {got_path}, not {spec['want']}"
    out, buf, margin = pb.launch()
    R.check_guard(buf, pb.M, pb.n_out, pb.ldc, margin, pb.dt, what=name)
    worst = pb.check(out, name)
    # identical bits from a second launch
    out2, _, _ = pb.launch()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), f"{name}: two launches differ"
    gn1 = pb.gn
    if pb.kind == "conv_gn":
        # the pair statistics: the fp64 sums of the stored output; and the same bits from the in-register fold (the GNS epilogue)
        o = out.double().view(pb.M // 128, 128, pb.N // 2, 2)
        s1, s2 = o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))
        a1, a2 = o.abs().sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))
        assert ((gn1[..., 0].double() - s1).abs() <= 1e-5 * a1 + 1e-6).all(), f"{name}: pair sums"
        assert ((gn1[..., 1].double() - s2).abs() <= 1e-5 * a2 + 1e-6).all(), f"{name}: pair sums of squares"
        assert pb.path(cus, splits=-pb.splits) == ("igemm128", 128, True, 1)
        out3, buf3, _ = pb.launch(splits=-pb.splits)
        R.check_guard(buf3, pb.M, pb.n_out, pb.ldc, margin, pb.dt, what=name + " fold")
        assert torch.equal(out.view(torch.int16), out3.view(torch.int16)) and torch.equal(gn1, pb.gn), f"{name}: split-K vs fold"
    # persistent kernels: the one-shot kernel of the same launch (test flag 8) gives the same bits
    if got_path[0] in ("pgemm", "pconv"):
        assert pb.path(cus, flags=8)[0] not in ("pgemm", "pconv")
        _lib.check(lib.hedit_test_set_flags(8))
        try:
            out8, buf8, _ = pb.launch()
        finally:
            _lib.check(lib.hedit_test_set_flags(0))
        R.check_guard(buf8, pb.M, pb.n_out, pb.ldc, margin, pb.dt, what=name + " one-shot")
        assert torch.equal(out.view(torch.int16), out8.view(torch.int16)), f"{name}: persistent and one-shot kernels differ"
    # batch invariance across a path boundary: the first tile / image alone
    if pb.kind != "conv_gn":
        ms = _small_rows(pb)
        if ms < pb.M and pb.path(cus, M=ms) != got_path:
            small, sbuf, smargin = pb.launch(M=ms)
            R.check_guard(sbuf, ms, pb.n_out, pb.ldc, smargin, pb.dt, what=name + " small")
            assert torch.equal(out[:ms].view(torch.int16), small.view(torch.int16)), \
                f"{name}: rows 0..{ms - 1} differ between {got_path} and {pb.path(cus, M=ms)} alone"
    print(f"gemm path {name}: {got_path}, M = {pb.M}, worst pointwise margin {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------- the linear M-sweep
# (N, K, tokens per image) of SD-1.5 linear layers: the canonical chunking is a function of N, K and tokens x GEMM_NOMINAL_BATCH (4)
SWEEP = [(320, 320, 4096), (1280, 1280, 64), (640, 2560, 1024), (1280, 5120, 256)]


def _run_gemm_splits(lib, M, N, K, chunk):
    """the split argument of hedit_k_gemm that executes the canonical chunking the way unet.hip::run_gemm does"""
    kt = K // BK
    s = lib.hedit_k_gemm_plan_splits(M, N, K, chunk)
    if s > 1:
        assert cdiv(kt, s) == chunk
        return s
    if chunk == 0:
        return 0
    f = cdiv(kt, chunk)
    assert cdiv(kt, f) == chunk
    return -f


def _sweep_rows(cus, N, K, chunk, lib):
    bn = pick_bn(N)
    tn = cdiv(N, bn)
    ms = {1, 5, 77, 127, 128, 129}

    def first(pred, lo=1, hi=1 << 20):          # smallest M with pred(M)  (pred monotone)
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(mid):
                hi = mid
            else:
                lo = mid + 1
        return lo
    splits = (lambda m: lib.hedit_k_gemm_plan_splits(m, N, K, chunk))      # noqa: E731
    for pred in (lambda m: cdiv(m, 128) * tn * splits(m) > cus,            # blocks of the 128-row tile past the CU count
                 lambda m: cdiv(m, 256) * tn >= 200,                       # the 256-row tile
                 lambda m: cdiv(m, 256) * tn >= 2 * cus):                  # the persistent kernel
        m = first(pred)
        ms |= {m - 1, m, m + 1}
    return sorted(x for x in ms if x >= 1)


@pytest.mark.parametrize("N,K,tokens", SWEEP, ids=[f"N{n}-K{k}" for n, k, _ in SWEEP])
def test_linear_rows_do_not_depend_on_the_launch(lib, cus, N, K, tokens):
    chunk = lib.hedit_k_gemm_canonical_chunk(tokens * 4, N, K)
    Ms = _sweep_rows(cus, N, K, chunk, lib)
    Mmax = Ms[-1]
    dt = _lib.storage_dtype()
    g = torch.Generator(device=DEV).manual_seed(N + K)
    A = torch.randn(Mmax, K, generator=g, device=DEV).to(dt)
    W = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(dt)
    bias = torch.randn(N, generator=g, device=DEV)
    res = torch.randn(Mmax, N, generator=g, device=DEV).to(dt)
    p = _lib.ptr
    outs, paths = {}, {}
    for M in Ms:
        sp = _run_gemm_splits(lib, M, N, K, chunk)
        paths[M] = path(cus, M, N, K, splits=sp, res=True)
        out = torch.empty(M, N, dtype=dt, device=DEV)
        ws = torch.empty(max(lib.hedit_k_gemm_ws_bytes(M, N, K, sp), 16), dtype=torch.uint8, device=DEV)
        _lib.check(lib.hedit_k_gemm(p(A), p(W), p(bias), p(res), p(out), M, N, K, K, N, N, 0, 0, 0, 0, 0, 0, sp, p(ws), None))
        outs[M] = out
    torch.cuda.synchronize()
    big = outs[Mmax]
    # the largest launch is itself right (pointwise on its first and last tile and a sample)
    rows = R.sample_rows(Mmax, n_random=512, seed=K).to(DEV)
    dot, mag = R.contract(A[rows], W)
    ref, pre, acc = R.reference(dot, mag, bias, res[rows])
    R.check_pointwise(big[rows], ref, pre, acc, K, dt, rows=rows, tile=(256, pick_bn(N)), what=f"sweep N {N} K {K} M {Mmax}")
    for M in Ms[:-1]:
        assert torch.equal(outs[M].view(torch.int16), big[:M].view(torch.int16)), \
            f"N {N} K {K}: rows of the M = {M} launch ({paths[M]}) differ from the M = {Mmax} launch ({paths[Mmax]})"
    kinds = {pt[0] for pt in paths.values()}
    want = {"igemm128deep"} | ({"igemm256"} if K // BK >= 16 else set()) | ({"pgemm"} if chunk == 0 else set())
    assert want <= kinds, f"N {N} K {K} chunk {chunk}: the sweep reached {sorted(kinds)} only"
    if chunk:
        assert any(pt[3] > 1 for pt in paths.values()) and any(pt[2] for pt in paths.values()), paths
    print(f"sweep N {N} K {K} chunk {chunk}: M {Ms} -> {sorted(kinds)}")

