"""The face task's Edit Friendly mode on the CPU: the PRODUCT's loop (hedit/inversion/ef_face.py, pure torch around a
differentiable callable) and its fp32 restatement (tests/helpers/face_ef_ref.py), both on the pinned CPU restatement of
the pixel UNet with plain autograd, against vectors produced by running the reference's face-swapping/inversion/ef.py
(tests/golden/make_golden_face_ef.py, g21) -- no GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.face_ef_ref import ef_ref  # noqa: E402
from helpers.tiny import TinyIdLoss, TinyLpips  # noqa: E402
from test_oracle_face import G11, face_state_dict, linear_betas  # noqa: E402
from oracle import ddpm_unet  # noqa: E402
from hedit.inversion.ef_face import ef  # noqa: E402

torch.set_num_threads(4)
G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_face_ef.npz")
T = 10
SEQ = (np.arange(0, 1000, 1000 // T) + 1)[::-1]
# name, skip, identity, LPIPS, mask
CASES = [("ef_s6", 6, True, True, False), ("ef_s6_idmask", 6, True, False, True), ("ef_s6_lp", 6, False, True, False),
         ("ef_s7_mask", 7, True, True, True), ("ef_s8", 8, True, True, False)]


@pytest.fixture(scope="module")
def model():
    m = ddpm_unet.Model(**ddpm_unet.TINY_DDPM).eval()
    m.load_state_dict(face_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@pytest.fixture(scope="module")
def inv():
    v = np.load(G11)
    return torch.from_numpy(v["zs"]), torch.from_numpy(v["xts"]), torch.from_numpy(v["mask"])


def run(fn, model, inv, skip, use_id, use_lp, use_mask, **kw):
    zs, xts, mask = inv
    after = T - skip
    return fn(model, TinyLpips() if use_lp else None, TinyIdLoss() if use_id else None, xts[after].clone(), linear_betas(), SEQ,
              eta=1.0, zs=zs[:after], weight_edit_face=100.0, after_skip_steps=after, num_inference_steps=T,
              soft_face_mask=mask if use_mask else None, **kw)


@pytest.mark.parametrize("fn", [ef, ef_ref], ids=["product", "restatement"])
@pytest.mark.parametrize("name,skip,use_id,use_lp,use_mask", CASES, ids=[c[0] for c in CASES])
def test_ef_matches_reference(model, inv, fn, name, skip, use_id, use_lp, use_mask):
    want = np.load(G21)[name]
    out = run(fn, model, inv, skip, use_id, use_lp, use_mask)
    assert out.shape == (1, 3, 32, 32) and out.requires_grad
    assert np.allclose(out.detach().numpy(), want, atol=5e-4, rtol=1e-4)      # the limits of test_oracle_face.py


def test_returns_the_sample_before_the_last_update(model, inv):
    """ef.py:81-82, :114: the loop breaks at tm1 == 0 before xt is replaced, so the result is the xt the LAST iteration
    started from -- the output of a run that stops one step earlier and takes its update"""
    after = 4
    trace = []
    out = run(ef_ref, model, inv, T - after, True, True, False, trace=trace)
    assert len(trace) == after and torch.equal(out.detach(), trace[-1])
    got = run(ef, model, inv, T - after, True, True, False)
    assert np.allclose(got.detach().numpy(), trace[-1].numpy(), atol=5e-4, rtol=1e-4)
    # a run that stops one step earlier starts its last iteration from the sample before that one
    shorter = []
    run(ef_ref, model, inv, T - after + 1, True, True, False, trace=shorter)
    assert len(shorter) == after - 1


def test_mask_reaches_only_the_identity_term(model, inv):
    _, _, mask = inv
    zero = torch.zeros_like(mask)
    # a zero mask removes the identity step: identity + LPIPS under it == LPIPS alone ...
    a = run(ef, model, inv, 7, True, True, False)
    both0 = ef(model, TinyLpips(), TinyIdLoss(), inv[1][3].clone(), linear_betas(), SEQ, zs=inv[0][:3], after_skip_steps=3,
               num_inference_steps=T, soft_face_mask=zero)
    lp_only = run(ef, model, inv, 7, False, True, False)
    assert torch.allclose(both0, lp_only, atol=1e-6)
    # ... and LPIPS alone does not see the mask at all
    lp_masked = ef(model, TinyLpips(), None, inv[1][3].clone(), linear_betas(), SEQ, zs=inv[0][:3], after_skip_steps=3,
                   num_inference_steps=T, soft_face_mask=zero)
    assert torch.equal(lp_masked, lp_only)
    assert (a - lp_only).abs().max() > 1e-3


def test_per_image_lockstep_equals_single_runs(model, inv):
    zs, xts, _ = inv
    after = 3
    x1, z1 = xts[after].reshape(1, 3, 32, 32), zs[:after].reshape(after, 1, 3, 32, 32)
    x2 = torch.cat([x1, x1.flip(-1) * 0.9])
    z2 = torch.cat([z1, z1.flip(-1)], 1)
    kw = dict(eta=1.0, weight_edit_face=100.0, after_skip_steps=after, num_inference_steps=T)
    both = ef(model, TinyLpips(), TinyIdLoss(), x2, linear_betas(), SEQ, zs=z2, per_image=True, **kw)
    for i in range(2):
        one = ef(model, TinyLpips(), TinyIdLoss(), x2[i:i + 1], linear_betas(), SEQ, zs=z2[:, i:i + 1], **kw)
        assert torch.allclose(both[i:i + 1], one, atol=2e-5, rtol=1e-5), i
    assert (both[0] - both[1]).abs().max() > 1e-2


def test_driver_accepts_the_ef_mode():
    import main_edit_face
    import main_edit_face_ef
    args = main_edit_face.build_parser().parse_args(["--mode", "ef"])
    assert args.mode == "ef"
    assert "main_edit_face_ef.py" in main_edit_face.build_parser().format_help()
    assert callable(main_edit_face_ef.main)
