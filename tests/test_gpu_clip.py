"""-m gpu: the native style encoder (hedit_vit_gram / hedit_vit_gram_fwd_bwd, csrc/vit.hip on the shared encoder kernels of
csrc/encoder.hip -- SURVEY.md section 8 row
a19) against (1) vectors produced by RUNNING the reference's CLIPEncoder.get_gram_matrix_residual and CLIP ViT
(text-guided-n-style/clip_guidance/base_clip.py, clip/model.py) at toy width, tests/golden/g10_clip.npz, and (2) the
oracle's fp32 restatement (oracle/reward_nets.py, pinned on the same vectors, run on the CPU) at ViT-B/16 shape.  Tolerances: fp32 token stream with 16 mantissa bits per GEMM operand and fp32
accumulation -> Gram residual / loss to 1e-4 relative, image gradient to 2e-3 relative L2 (the reference itself runs
this encoder in fp16, model.py:414-435)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from helpers import gpu as G  # noqa: E402
from oracle import reward_nets as RN  # noqa: E402
from helpers.tiny import hash_normal  # noqa: E402
from test_host_clip import G10, toy_prefix  # noqa: E402
from hedit.clip_guidance import CLIPEncoder  # noqa: E402
from hedit.clip_guidance.base_clip import ClipVisualPrefix  # noqa: E402


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    g = np.load(G10)
    path = str(tmp_path_factory.mktemp("style") / "ref.png")
    Image.fromarray(g["ref_rgb"]).save(path)
    return CLIPEncoder(need_ref=True, ref_path=path, clip_model=toy_prefix(), device=G.dev()), g


@pytest.mark.parametrize("i,hw", [(0, (64, 64)), (1, (96, 80))])
def test_native_gram_residual_and_gradient_match_reference_vectors(enc, i, hw):
    e, g = enc
    im = G.f32(hash_normal((1, 3) + hw, 900 + i) * 0.6).requires_grad_(True)
    res = e.get_gram_matrix_residual(im.detach())
    G.sync()
    assert res.shape == (64, 64)
    assert G.rel_err(res, torch.from_numpy(g[f"residual{i}"])) < 1e-4
    loss = e.gram_residual_norms(im).sum()
    (grad,) = torch.autograd.grad(loss, im)
    G.sync()
    assert abs(loss.item() - g[f"loss{i}"][0]) < 1e-4 * g[f"loss{i}"][0]
    assert G.rel_err(grad, torch.from_numpy(g[f"grad{i}"])) < 2e-3
    # the reference's own call pattern: the residual MATRIX under autograd, then torch.linalg.norm (h_edit.py:172-175)
    im2 = im.detach().clone().requires_grad_(True)
    (grad2,) = torch.autograd.grad(torch.linalg.norm(e.get_gram_matrix_residual(im2)), im2)
    G.sync()
    assert G.rel_err(grad2, torch.from_numpy(g[f"grad{i}"])) < 2e-3
    # ... and an arbitrary linear functional of it (upstream gradient that is not the norm's)
    u = G.f32(hash_normal((64, 64), 5 + i))
    im3 = im.detach().clone().requires_grad_(True)
    (grad3,) = torch.autograd.grad((e.get_gram_matrix_residual(im3) * u).sum(), im3)
    imc = im.detach().cpu().clone().requires_grad_(True)
    ec = _cpu_twin(e)
    (want3,) = torch.autograd.grad((RN.clip_gram_residual(ec, imc) * u.cpu()).sum(), imc)
    G.sync()
    assert G.rel_err(grad3, want3) < 2e-3


def _cpu_twin(e):
    """the same parameters and style reference on the CPU, for the oracle"""
    import copy
    twin = CLIPEncoder(clip_model=copy.deepcopy(e.clip_model).cpu().float())
    twin.set_reference(e.ref.detach().cpu().float())
    return twin


def test_native_matches_oracle_at_vit_b16_shape_and_is_batch_invariant():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m = ClipVisualPrefix().init_random(13)
    ref = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(17))
    nat = CLIPEncoder(clip_model=m.float(), device=G.dev())
    nat.set_reference(ref.to(G.dev()))
    tor = _cpu_twin(nat)
    ims = torch.randn(4, 3, 512, 512, generator=torch.Generator().manual_seed(3)) * 0.5
    xn, xt = G.f32(ims).requires_grad_(True), ims.clone().requires_grad_(True)
    ln, lt = nat.gram_residual_norms(xn), RN.clip_gram_residual_norms(tor, xt)
    gn, gt = torch.autograd.grad(ln.sum(), xn)[0], torch.autograd.grad(lt.sum(), xt)[0]
    G.sync()
    assert G.rel_err(ln, lt) < 1e-4
    assert G.rel_err(gn, gt) < 2e-3
    one = nat.gram_residual_norms(G.f32(ims[2:3]))
    G.sync()
    assert torch.equal(one, ln[2:3].detach())


def test_residual_matrix_backward_at_vit_b16_scale():
    """The residual MATRIX under autograd with an upstream gradient that is NOT the norm's (get_gram_matrix_residual,
    gram_residuals: the reference's call pattern, h_edit.py:172-175) at ViT-B/16 width, where the Gram entries are
    1e2...1e4 and a unit-norm U has entries of 1e-3: the backward hands the executor Gram - s U with s a power of two of
    the order |Gram|max / |U|max, so U survives the subtraction (unscaled it was quantised to half an ulp of Gram --
    ADVICE round 3).  Measured: relative L2 error of the image gradient vs the fp32 oracle on the CPU (autograd) well
    below the 2e-3 the norm path is held to."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m = ClipVisualPrefix().init_random(13)
    ref = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(17))
    nat = CLIPEncoder(clip_model=m.float(), device=G.dev())
    nat.set_reference(ref.to(G.dev()))
    tor = _cpu_twin(nat)
    im = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(5)) * 0.5
    u = torch.randn(768, 768, generator=torch.Generator().manual_seed(6))
    u = u / u.norm()
    xn, xt = G.f32(im).requires_grad_(True), im.clone().requires_grad_(True)
    res = nat.get_gram_matrix_residual(xn)
    (gn,) = torch.autograd.grad((res * G.f32(u)).sum(), xn)
    (gt,) = torch.autograd.grad((RN.clip_gram_residual(tor, xt) * u).sum(), xt)
    G.sync()
    assert float(res.detach().abs().max()) > 50.0          # the regime the rescaling exists for
    err = G.rel_err(gn, gt)
    print(f"residual-matrix backward at ViT-B/16 scale: rel L2 err {err:.3e}")
    assert err < 2e-3


def test_there_is_no_cpu_path():
    e = CLIPEncoder(clip_model=toy_prefix())
    e.set_reference(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        e.gram_residual_norms(torch.zeros(1, 3, 64, 64))
