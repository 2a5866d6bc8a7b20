"""-m gpu: the one-launch GroupNorm of images below 32 x 32 (csrc/norm.hip).  gn_small_kernel (wide vectors through LDS, a 1-D grid
that keeps the groups of an image on one XCD) must give the bits of its kept first form gn_small_narrow_kernel (4 bytes per lane,
grid (group, image); hedit_test_set_flags bit 4) -- y and (mean, rstd) alike --, for every vector width, with and without SiLU, with
and without the statistics output, at batch sizes that leave empty tail blocks in the padded grid (3 and 9: not multiples of 8).
Inputs carry a per-channel offset of a few units, so another summation order would move the statistics' last bits."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import gpu as G  # noqa: E402
from hedit import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
# (HW, C, groups): 16-byte vectors / the 160-byte slice and the largest LDS image / 120-byte slice, 8-byte vectors / 40-byte slice /
# two channels a group: one pair per pixel, 4-byte path / 16 bytes with 16 groups
SHAPES = [(64, 1280, 32), (256, 2560, 32), (256, 1920, 32), (256, 640, 32), (16, 64, 32), (64, 128, 16)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.lib()


def make(B, HW, C):
    g = torch.Generator().manual_seed(HW * 7 + C + B)
    x = torch.randn(B, HW, C, generator=g) * 1.5 + 3.0 * torch.randn(C, generator=g)
    return G.bf(x), G.f32(1 + 0.1 * torch.randn(C, generator=g)), G.f32(0.1 * torch.randn(C, generator=g))


def run(lib, x, gamma, beta, Gn, silu, with_stats, kept):
    """y (and stats) of one launch; kept = the narrow kernel"""
    B, HW, C = x.shape
    y = torch.full_like(x, 7.0)
    stats = torch.full((B, Gn, 2), -1.0, dtype=torch.float32, device=G.dev()) if with_stats else None
    ws = torch.empty(max(lib.hedit_k_groupnorm_ws_bytes(B, HW, C), 16), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.hedit_test_set_flags(16 if kept else 0))
    try:
        if with_stats:
            _lib.check(lib.hedit_k_groupnorm_stats(_lib.ptr(x), _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), B, HW, C, Gn, EPS, silu,
                                                   _lib.ptr(ws), _lib.ptr(stats), None))
        else:
            _lib.check(lib.hedit_k_groupnorm(_lib.ptr(x), _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), B, HW, C, Gn, EPS, silu,
                                             _lib.ptr(ws), None))
        G.sync()
    finally:
        _lib.check(lib.hedit_test_set_flags(0))
    return y, stats


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("HW,C,Gn", SHAPES)
def test_wide_kernel_gives_the_narrow_kernels_bits(lib, HW, C, Gn, B):
    x, gamma, beta = make(B, HW, C)
    for silu in (0, 1):
        for with_stats in (False, True):
            y_new, st_new = run(lib, x, gamma, beta, Gn, silu, with_stats, kept=False)
            y_old, st_old = run(lib, x, gamma, beta, Gn, silu, with_stats, kept=True)
            assert torch.equal(y_new, y_old), (silu, with_stats)
            if with_stats:
                assert torch.equal(st_new, st_old), silu
                assert (st_new[..., 1] > 0).all()          # every (image, group) was written


def test_unaligned_base_takes_a_narrower_vector_and_keeps_the_bits(lib):
    """a tensor that starts 8 bytes (4 elements) past a 16-byte boundary: the 16-byte slices of C = 1280 go in 8-byte vectors"""
    B, HW, C = 3, 64, 1280
    x, gamma, beta = make(B, HW, C)
    buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=G.dev())
    xo = buf[4:].view(B, HW, C)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 8
    y_al, st_al = run(lib, x, gamma, beta, 32, 1, True, kept=False)
    y_un, st_un = run(lib, xo, gamma, beta, 32, 1, True, kept=False)
    assert torch.equal(y_al, y_un) and torch.equal(st_al, st_un)


@pytest.mark.parametrize("HW,C,Gn", [(256, 1920, 32), (64, 1280, 32)])
def test_against_fp64_groupnorm(lib, HW, C, Gn):
    x, gamma, beta = make(9, HW, C)
    y, stats = run(lib, x, gamma, beta, Gn, 1, True, kept=False)
    xd = x.double().permute(0, 2, 1)
    want = F.silu(F.group_norm(xd, Gn, gamma.double(), beta.double(), eps=EPS)).permute(0, 2, 1)
    G.within(G.rel_err(y, want), 5e-3, what="gn_small")
    mean = xd.reshape(9, Gn, -1).mean(-1)
    assert (stats[..., 0].double() - mean).abs().max().item() < 1e-4


@pytest.mark.parametrize("HW,C,Gn", [(256, 1280, 32), (256, 640, 32), (16, 64, 32)])
def test_an_image_alone_equals_the_image_in_a_batch(lib, HW, C, Gn):
    x, gamma, beta = make(9, HW, C)
    y9, st9 = run(lib, x, gamma, beta, Gn, 1, True, kept=False)
    y1, st1 = run(lib, x[2:3].contiguous(), gamma, beta, Gn, 1, True, kept=False)
    assert torch.equal(y9[2:3], y1) and torch.equal(st9[2:3], st1)


@pytest.mark.skipif(G.F16, reason="this IS the half-storage run")
def test_the_file_passes_in_half_storage():
    """one storage format per process (hedit/_lib.py): the same comparisons on libhedit_hip_f16.so, in a child pytest"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, HEDIT_STORAGE="f16")
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", os.path.basename(__file__)), "-q", "-x", "--tb=short",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "18 passed" in out and "1 skipped" in out, out[-500:]
