"""The native face-parsing network and soft face mask (csrc/faceparse.hip, hedit.arcface.FaceParsing / face_mask) against
vectors produced by RUNNING the reference's FaceParsing, encode_segmentation and SoftErosion with hash-seeded weights:
tests/golden/g17_face_parsing.{npz,json}, generator tests/golden/make_golden_parsing.py.  Then the face driver's
post-processing with the network's checkpoint in ./arcface/weights (main_edit.py:120-127, :184-191, :211-212)."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.parsing import parsing_state_dict  # noqa: E402
from hedit.arcface import FaceParsing, face_mask  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_face_parsing")
META = json.load(open(GOLD + ".json"))
CASES = [c["name"] for c in META["cases"]]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD + ".npz"))


@pytest.fixture(scope="module")
def net():
    m = FaceParsing(device="cuda:0")
    m.load_state_dict(parsing_state_dict({k: tuple(s) for k, s in META["params"]}))
    return m


def _image(gold, name):
    rgb = torch.from_numpy(gold[f"{name}_rgb"])
    return (rgb.permute(2, 0, 1).float().div(255) * 2 - 1).unsqueeze(0).cuda()


def _margin_tol(name):
    # 1e-4 at torch's default init (logits ~0.3), scaled to the logit spread of the hash-seeded weights
    std = next(c["logit_std"] for c in META["cases"] if c["name"] == name)
    return 1e-4 * max(1.0, std / 0.3)


def test_native_parameter_table_is_the_reference_one():
    from hedit import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(lib.hedit_faceparse_create(ctypes.byref(h)))
    try:
        nd, dims = ctypes.c_int(), (ctypes.c_int * 4)()
        table = []
        for i in range(lib.hedit_faceparse_num_params(h)):
            _lib.check(lib.hedit_faceparse_param_shape(h, i, ctypes.byref(nd), dims))
            table.append([lib.hedit_faceparse_param_name(h, i).decode(), [dims[k] for k in range(nd.value)]])
        assert lib.hedit_faceparse_missing(h) == len(table)
    finally:
        lib.hedit_faceparse_destroy(h)
    assert table == [p for p in META["params"] if not p[0].endswith("num_batches_tracked")]


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", CASES)
def test_labels_match_reference(gold, net, name, mode):
    """every pixel whose top-1 - top-2 margin is not tiny, and >= 99.9 % of all pixels"""
    net.train(mode == "train")
    try:
        lab = net(_image(gold, name))
    finally:
        net.train()
    sfx = "" if mode == "train" else "_eval"
    ref = torch.from_numpy(gold[f"{name}_labels{sfx}"].astype(np.int64))
    margin = torch.from_numpy(gold[f"{name}_margin{sfx}"])
    assert lab.dtype == torch.int64 and lab.shape == (1, 1) + tuple(ref.shape)
    diff = lab[0, 0].cpu() != ref
    assert not diff[margin >= _margin_tol(name)].any(), int(diff[margin >= _margin_tol(name)].sum())
    assert diff.float().mean().item() <= 1e-3, diff.float().mean().item()


@pytest.mark.parametrize("name", CASES)
def test_mask_matches_reference(gold, name):
    labels = torch.from_numpy(gold[f"{name}_labels"].astype(np.int64))[None, None].cuda()
    soft, hard = face_mask(labels)
    assert soft.dtype == torch.float32 and hard.dtype == torch.bool and soft.shape == hard.shape == labels.shape
    field = torch.from_numpy(gold[f"{name}_field"])
    decided = (field - META["threshold"]).abs() > 1e-5       # 0 outside the stored band: decided
    ref_soft, ref_hard = torch.from_numpy(gold[f"{name}_soft"]), torch.from_numpy(gold[f"{name}_hard"]).bool()
    s, hd = soft[0, 0].cpu(), hard[0, 0].cpu()
    assert torch.equal(hd[decided], ref_hard[decided])
    assert (s - ref_soft)[decided].abs().max().item() <= 1e-5


def test_batch_invariance(gold, net):
    """one batch [a, b, a] == each image alone, bit for bit (BatchNorm statistics per image, not pooled over the batch)"""
    a, b = _image(gold, CASES[0]), _image(gold, CASES[1])
    lab = net(torch.cat([a, b, a]))
    la, lb = net(a), net(b)
    assert torch.equal(lab[0:1], la) and torch.equal(lab[1:2], lb) and torch.equal(lab[2:3], la)
    soft, hard = face_mask(lab)
    for k, single in ((0, la), (1, lb), (2, la)):
        s1, h1 = face_mask(single)
        assert torch.equal(soft[k:k + 1], s1) and torch.equal(hard[k:k + 1], h1)


def test_repeatable_and_degenerate(gold, net):
    x = _image(gold, CASES[2])
    l1, l2 = net(x), net(x)
    assert torch.equal(l1, l2)
    s1, h1 = face_mask(l1)
    s2, h2 = face_mask(l2)
    assert torch.equal(s1, s2) and torch.equal(h1, h2)
    # no face pixel: the maximum below the threshold is 0 -> soft 0 (the reference divides 0 by 0)
    soft, hard = face_mask(torch.zeros(2, 1, 48, 32, dtype=torch.int64, device="cuda"))
    assert not torch.isnan(soft).any() and (soft == 0).all() and not hard.any()
    # every pixel hard (mouth counts 2; one blur of a 3 x 3 cone keeps even the corners above 0.9): soft 1 everywhere
    soft, hard = face_mask(torch.full((1, 1, 16, 16), 10, dtype=torch.int64, device="cuda"), kernel_size=3, iterations=1)
    assert (soft == 1).all() and hard.all()
    # all face: hard interior, a rim below the threshold normalised by its own maximum
    soft, hard = face_mask(torch.ones(1, 1, 64, 64, dtype=torch.int64, device="cuda"))
    assert not torch.isnan(soft).any() and hard.any() and not hard.all()
    assert soft[~hard].max().item() == 1.0 and (soft[hard] == 1).all()


def _driver():
    spec = importlib.util.spec_from_file_location("hedit_main_face_parsing", os.path.join(ROOT, "h-edit_amd", "main_edit_face.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_face_driver_blends_through_the_parsing_network(tmp_path, monkeypatch):
    """./arcface/weights/face_parsing.pth present, no --mask_dir: the sheet's result is edited * soft + source * (1 - soft)
    with the mask of the network on the source; --batch 2 writes the same bytes as the pair-by-pair run."""
    from PIL import Image
    from hedit.arcface.arcface_model import load_face_image
    from hedit.utils import image_grid
    drv = _driver()
    d = tmp_path / "faces"
    d.mkdir()
    y, x = np.mgrid[0:80, 0:72]
    for i, name in enumerate(("a.jpg", "b.jpg", "c.jpg")):
        Image.fromarray(np.stack([(x * (i + 2)) % 256, (y * 3 + i * 40) % 256, (x + y * (i + 1)) % 256], -1).astype(np.uint8)).save(d / name)
    with open(d / "demo.json", "w") as f:
        json.dump([dict(idx=0, ref="a.jpg", source="b.jpg"), dict(idx=1, ref="c.jpg", source="a.jpg")], f)
    sd = parsing_state_dict({k: tuple(s) for k, s in META["params"]})
    (tmp_path / "arcface" / "weights").mkdir(parents=True)
    torch.save(sd, tmp_path / "arcface" / "weights" / "face_parsing.pth")
    monkeypatch.chdir(tmp_path)
    edited = []
    real = drv.h_Edit_R

    def spy(*a, **k):
        out = real(*a, **k)
        edited.append(out.detach().clone())
        return out
    monkeypatch.setattr(drv, "h_Edit_R", spy)
    common = ["--json_file", str(d / "demo.json"), "--image_path", str(d) + "/", "--random_init", "--tiny", "--no_lpips",
              "--num_diffusion_steps", "10", "--optimization_steps", "2", "--weight_edit_face", "4.0"]
    one = drv.main(common + ["--output_path", str(tmp_path / "o1") + "/"])
    assert len(one) == 2 and len(edited) == 2
    net = FaceParsing(device="cuda:0")
    net.load_state_dict(sd)
    for k, (ref_name, src_name) in enumerate((("a.jpg", "b.jpg"), ("c.jpg", "a.jpg"))):
        src = load_face_image(str(d / src_name), 32).cuda()
        ref = load_face_image(str(d / ref_name), 32)
        soft, _ = face_mask(net(src))
        assert 0 < soft.mean().item() < 1
        want = image_grid([ref, src.cpu(), (edited[k] * soft + src * (1 - soft)).cpu()])
        got = [p for p in one if p.endswith(f"item_{ref_name[0]}_{src_name[0]}.png")]
        assert len(got) == 1 and np.array_equal(np.array(Image.open(got[0])), np.array(want))
        unblended = np.array(image_grid([ref, src.cpu(), edited[k].cpu()]))
        assert not np.array_equal(np.array(Image.open(got[0])), unblended)
    two = drv.main(common + ["--output_path", str(tmp_path / "o2") + "/", "--batch", "2"])
    assert len(two) == 2
    for a, b in zip(sorted(one), sorted(two)):
        assert os.path.basename(a) == os.path.basename(b)
        assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b)))
