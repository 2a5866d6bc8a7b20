"""-m gpu: the face task's Edit Friendly mode (hedit/inversion/ef_face.py) on the HIP eps-network with its input-gradient pass
(hedit.diffusion.Model(grad=True)), against the fp32 restatement of the reference's loop (tests/helpers/face_ef_ref.py,
pinned on vectors from running face-swapping/inversion/ef.py: tests/test_host_face_ef.py, g21) on the oracle model.

The yardstick is computed here from reference-side code only: the same restatement with the oracle under bf16 autocast.
Limit = 2 x that error -- autocast rounds the operands of convolutions and matrix products only, the executor also stores
every activation and every gradient in 16 bits.  Each case first shows that it can see the UNet's Jacobian at all: the
restatement with eps detached (the gradient through the eps-network cut) is at least 3 x the limit away from the true one."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers.face_ef_ref import autocast_bf16, ef_ref  # noqa: E402
from helpers.tiny import TinyIdLoss, TinyLpips, hash_normal  # noqa: E402
from test_oracle_face import G11, face_state_dict, linear_betas  # noqa: E402

pytestmark = pytest.mark.gpu

T = 10
SEQ = (np.arange(0, 1000, 1000 // T) + 1)[::-1]
# name, skip, identity, LPIPS, mask
CASES = [("ef_s6", 6, True, True, False), ("ef_s6_idmask", 6, True, False, True), ("ef_s6_lp", 6, False, True, False),
         ("ef_s7_mask", 7, True, True, True), ("ef_s8", 8, True, True, False)]


@functools.lru_cache(maxsize=None)
def models():
    """the HIP model with gradient and the oracle, on the weights the golden vectors were made with"""
    from hedit.diffusion import Model, TINY_DDPM_CONFIG
    from oracle import ddpm_unet
    om = ddpm_unet.Model(**ddpm_unet.TINY_DDPM).eval()
    sd = face_state_dict({k: tuple(v.shape) for k, v in om.state_dict().items()})
    om.load_state_dict(sd)
    for p in om.parameters():
        p.requires_grad_(False)
    hip = Model(TINY_DDPM_CONFIG, device=G.dev(), grad=True)
    hip.load_state_dict(sd)
    return hip, om


@functools.lru_cache(maxsize=None)
def inv():
    v = np.load(G11)
    return torch.from_numpy(v["zs"]), torch.from_numpy(v["xts"]), torch.from_numpy(v["mask"])


def kwargs(skip, use_mask, dev="cpu"):
    zs, xts, mask = inv()
    after = T - skip
    return dict(xT=xts[after].clone().to(dev), betas=linear_betas().to(dev), seq=SEQ, eta=1.0, zs=zs[:after].to(dev),
                weight_edit_face=100.0, after_skip_steps=after, num_inference_steps=T,
                soft_face_mask=mask.to(dev) if use_mask else None)


@functools.lru_cache(maxsize=None)
def references(name, skip, use_id, use_lp, use_mask):
    """(fp32 restatement, its bf16-autocast run, its run with the UNet Jacobian cut), all on the CPU oracle: computed once"""
    _, om = models()
    lp, idl = (TinyLpips() if use_lp else None), (TinyIdLoss() if use_id else None)
    want = ef_ref(om, lp, idl, **kwargs(skip, use_mask)).detach()
    auto = ef_ref(autocast_bf16(om), lp, idl, **kwargs(skip, use_mask)).detach()
    cut = ef_ref(om, lp, idl, detach_eps=True, **kwargs(skip, use_mask)).detach()
    return want, auto, cut


@pytest.mark.parametrize("name,skip,use_id,use_lp,use_mask", CASES, ids=[c[0] for c in CASES])
def test_ef_on_the_hip_model_matches_the_restatement(name, skip, use_id, use_lp, use_mask):
    from hedit.inversion.ef_face import ef
    hip, _ = models()
    dev = G.dev()
    want, auto, cut = references(name, skip, use_id, use_lp, use_mask)
    limit = 2.0 * G.rel_err(auto, want)
    sens = G.rel_err(cut, want)
    lp = TinyLpips().to(dev) if use_lp else None
    idl = TinyIdLoss().to(dev) if use_id else None
    kw = kwargs(skip, use_mask, dev)
    got = ef(hip, lp, idl, kw.pop("xT"), kw.pop("betas"), kw.pop("seq"), **kw)
    G.sync()
    err = G.rel_err(got, want)
    print(f"{name}: hip vs restatement {err:.3e}, limit (2 x bf16 autocast) {limit:.3e}, eps detached {sens:.3e}")
    assert got.shape == (1, 3, 32, 32) and torch.isfinite(got).all()
    assert sens >= 3.0 * limit, (sens, limit)            # the case sees the UNet's input gradient
    # half storage: the yardstick is bfloat16's, so the limit scales like every storage-caused one
    G.within(err, limit, what="face ef " + name)


def test_lockstep_faces_equal_single_runs():
    """ef(per_image=True) on two faces at once == the two single runs, bit for bit: the eps-network and its input gradient are
    batch-invariant, and so is everything between their evaluations (the stand-in rewards evaluate image by image, as in
    tests/test_gpu_face.py: torch picks its own kernels by batch size)."""
    from hedit.inversion.ef_face import ef
    hip, _ = models()
    dev = G.dev()
    n = 4
    seq = SEQ
    betas = linear_betas().to(dev)
    xT = (hash_normal((2, 3, 32, 32), 5) * 0.9).to(dev)
    zs = hash_normal((n, 2, 3, 32, 32), 6).to(dev)

    class PerImage(torch.nn.Module):
        def __init__(self, inner, method):
            super().__init__()
            self.inner = inner
            setattr(self, method, lambda x: torch.stack([getattr(inner, method)(x[j:j + 1]) for j in range(x.shape[0])]).mean())
    idl, lp = PerImage(TinyIdLoss().to(dev), "get_cosine_loss"), PerImage(TinyLpips().to(dev), "get_lpips_loss")
    kw = dict(eta=1.0, weight_edit_face=100.0, after_skip_steps=n, num_inference_steps=T)
    both = ef(hip, lp, idl, xT, betas, seq, zs=zs, per_image=True, **kw)
    for i in range(2):
        one = ef(hip, lp, idl, xT[i:i + 1], betas, seq, zs=zs[:, i:i + 1], **kw)
        G.sync()
        assert torch.equal(both[i:i + 1], one), i
    assert G.rel_err(both[0], both[1]) > 1e-1


def _demo_files(tmp_path):
    import json
    from PIL import Image
    rng = np.random.RandomState(0)
    for n in ("a.png", "b.png"):
        Image.fromarray(rng.randint(0, 255, (32, 32, 3), dtype=np.uint8)).save(tmp_path / n)
    (tmp_path / "pairs.json").write_text(json.dumps([{"idx": 0, "source": "a.png", "ref": "b.png"}]))


def test_driver_ef_mode_writes_its_image(tmp_path):
    import main_edit_face_ef
    from PIL import Image
    _demo_files(tmp_path)
    out = str(tmp_path / "out") + "/"
    written = main_edit_face_ef.main(["--mode", "ef", "--random_init", "--tiny", "--num_diffusion_steps", "10", "--skip", "6",
                                      "--json_file", str(tmp_path / "pairs.json"), "--image_path", str(tmp_path), "--output_path", out])
    assert len(written) == 1 and "/ef/steps_10_skip_6_" in written[0] and os.path.exists(written[0])
    assert Image.open(written[0]).size[0] > 0


def test_driver_still_refuses_other_modes(tmp_path):
    import main_edit_face
    import main_edit_face_ef
    for drv in (main_edit_face, main_edit_face_ef):
        with pytest.raises(NotImplementedError):
            drv.main(["--mode", "nonsense", "--random_init", "--tiny"])
    with pytest.raises(NotImplementedError):          # the EF driver runs ef only
        main_edit_face_ef.main(["--mode", "h_edit_R", "--random_init", "--tiny"])
