"""Mask-guided MasaCtrl, host side (no GPU): the fp64 restatement of the reference's two editors
(tests/helpers/masactrl_mask_ref.py) against vectors from running the reference's own classes (g28), the class-array
builder, the refusals, the plan's new fields and the driver's flag."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import masactrl_mask_ref as MR
from hedit import _lib
from hedit.masactrl import (MutualSelfAttentionControl, MutualSelfAttentionControlMask,
                            MutualSelfAttentionControlMaskAuto)
from hedit.masactrl.masactrl import block_resolutions, mask_classes
from hedit.unet import SD15_CONFIG, TINY_CONFIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS, D = 2, 2
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "g28_masactrl_mask.npz"))


def close(got, want):
    """the golden file keeps the two target rows (1, 3) of the reference's four"""
    got, want = got[[1, 3]], torch.from_numpy(want).double()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())     # the reference ran in fp32


# ------------------------------------------------------------------------------------------------ helper against the reference
@pytest.mark.parametrize("kind,N,seed", [("mixed", 64, 101), ("mixed", 256, 102), ("empty", 64, 103), ("empty", 256, 104)])
def test_helper_given_masks_match_the_reference(kind, N, seed):
    q, k, v = (t.double() for t in MR.golden_qkv(seed, HEADS, D, N))
    ms, mt = MR.golden_given_masks(kind, seed)
    res = int(N ** 0.5)
    masks = MR.at_resolution(ms.double(), res), MR.at_resolution(mt.double(), res)
    got = MR.editor_rows(q, k, v, D ** -0.5, masks)
    close(got, GOLDEN[f"given_{kind}_{N}"])
    if kind == "empty":       # no background key: the reference's fill absorbs the logits, the mean of V
        bg = masks[1] == 0
        mean_v = v[2].mean(dim=1)                                               # (h, d)
        assert (got[3][bg] - mean_v.reshape(1, -1)).abs().max().item() < 1e-12


@pytest.mark.parametrize("N,thres,ref_idx,cur_idx,seed", [(64, 0.1, [1], [1], 201), (256, 0.1, [1, 2], [3], 202), (256, 0.5, [2], [2], 203)])
def test_helper_auto_masks_match_the_reference(N, thres, ref_idx, cur_idx, seed):
    q, k, v = (t.double() for t in MR.golden_qkv(seed, HEADS, D, N))
    cross = [p.mean(1) for p in MR.golden_cross(seed, HEADS)]                   # fp32 like the reference: the same thresholded mask
    ms, mt, ns, nt = MR.auto_masks(cross, ref_idx, cur_idx, thres, int(N ** 0.5))
    assert 0 < ms.sum() < ms.numel() and 0 < mt.sum() < mt.numel()
    close(MR.editor_rows(q, k, v, D ** -0.5, (ms.double(), mt.double())), GOLDEN[f"auto_{N}_{thres}_{seed}"])


def test_helper_auto_without_maps_is_plain_mutual_attention():
    q, k, v = (t.double() for t in MR.golden_qkv(301, HEADS, D, 64))
    close(MR.editor_rows(q, k, v, D ** -0.5, None), GOLDEN["auto_nomap_64"])


def test_helper_constant_map_is_background():
    cross = [torch.full((4, 256, 77), 1.0 / 77)]
    ms, mt, ns, _ = MR.auto_masks(cross, [1], [1], 0.1, 16, constant_is_background=True)
    assert ms.sum() == 0 and mt.sum() == 0
    assert torch.isnan(MR.aggregate(cross, [1])).all()                          # what the reference has there


# ------------------------------------------------------------------------------------------------ class arrays
@pytest.mark.parametrize("res", [8, 16, 32, 64])
def test_class_arrays_are_nearest_interpolation(res):
    g = torch.Generator().manual_seed(res)
    m = (torch.rand(3, 48, 48, generator=g) < 0.4).float()
    got = mask_classes(m, res)
    assert got.dtype == torch.uint8 and got.shape == (3, res * res)
    want = F.interpolate(m[:, None], (res, res))[:, 0]
    assert torch.equal(got.reshape(3, res, res).float(), want)
    idx = torch.floor(torch.arange(res) * (48 / res)).long()                    # nearest: source index floor(dst * in / out)
    assert torch.equal(want, m[:, idx][:, :, idx])


def fake_unet(cfg):
    return types.SimpleNamespace(device=torch.device("cpu"), config=dict(cfg))


def test_block_resolutions_follow_the_unet():
    assert block_resolutions(fake_unet(SD15_CONFIG), 64) == [64, 64, 32, 32, 16, 16, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64]
    assert block_resolutions(fake_unet(TINY_CONFIG), 32) == [32, 32, 16, 16, 8, 16, 16, 16, 32, 32, 32]


def test_plan_carries_the_classes_only_on_active_steps():
    u = fake_unet(TINY_CONFIG)
    m = torch.zeros(2, 32, 32)
    m[0, 8:24, 8:24] = 1
    m[1, :, :16] = 1
    ed = MutualSelfAttentionControlMask(1, 2, mask_s=m, mask_t=m, keep_masks=True)
    p = ed._plan(u, 8, 32, 32, True)
    assert not p.kv_src and p.n_masa_rows == 0                                  # step 0 < start_step: today's plan
    ed._after_pass(True)
    p = ed._plan(u, 8, 32, 32, True)
    assert p.kv_src and p.kv_first_block == 2 and p.n_masa_rows == 4 and not p.masa_auto
    assert [p.h_masa_rows[i] for i in range(4)] == [2, 3, 6, 7]
    tokens = sorted(p.h_masa_tokens[i] for i in range(p.n_masa_res))
    assert tokens == [64, 256, 1024]
    src, tar = ed.saved_masks[(1, 2)]                                           # block 2: 16 x 16
    assert src.shape == (2, 16, 16) and torch.equal(src, mask_classes(m, 16).reshape(2, 16, 16))
    assert set(ed.saved_masks) == {(1, b) for b in range(2, 11)}
    plain = MutualSelfAttentionControl(1, 2)._plan(u, 8, 32, 32, True)
    assert plain.n_masa_rows == 0 and not plain.h_masa_cls_q


# ------------------------------------------------------------------------------------------------ refusals
def test_masks_must_be_binary_and_present():
    ok = torch.ones(8, 8)
    with pytest.raises(ValueError, match="0 and 1"):
        MutualSelfAttentionControlMask(mask_s=ok * 0.5, mask_t=ok)
    with pytest.raises(ValueError, match="0 and 1"):
        MutualSelfAttentionControlMask(mask_s=ok, mask_t=ok * 2)
    with pytest.raises(ValueError, match="mask_s is missing"):
        MutualSelfAttentionControlMask(mask_t=ok)
    with pytest.raises(ValueError, match="mask_t is missing"):
        MutualSelfAttentionControlMask(mask_s=ok)
    with pytest.raises(ValueError, match=r"\(h, w\) or \(n, h, w\)"):
        MutualSelfAttentionControlMask(mask_s=torch.ones(1, 1, 8, 8), mask_t=torch.ones(1, 1, 8, 8))
    with pytest.raises(ValueError, match="same shape"):
        MutualSelfAttentionControlMask(mask_s=ok, mask_t=torch.ones(4, 4))


@pytest.mark.parametrize("make", [lambda: MutualSelfAttentionControlMask(0, 0, mask_s=torch.ones(8, 8), mask_t=torch.ones(8, 8)),
                                  lambda: MutualSelfAttentionControlMaskAuto(0, 0)])
def test_passes_without_the_four_row_layout_are_refused_by_name(make):
    u = fake_unet(TINY_CONFIG)
    with pytest.raises(NotImplementedError, match="non-square"):
        make()._plan(u, 4, 32, 64, True)
    with pytest.raises(NotImplementedError, match="MutualSelfAttentionControlMask.* 4n-row"):
        make()._plan(u, 2, 32, 32, True, n_images=1)           # the 2n-row passes of the baselines / Plug-and-Play loops
    with pytest.raises(ValueError, match="rows"):
        make()._plan(u, 6, 32, 32, True)
    with pytest.raises(RuntimeError, match="inside the HIP attention kernels"):
        make()(None, False, "down")                           # not a host-language (foreign) controller


def test_wrong_number_of_masks_is_refused():
    ed = MutualSelfAttentionControlMask(0, 0, mask_s=torch.ones(3, 8, 8), mask_t=torch.ones(3, 8, 8))
    with pytest.raises(ValueError, match="3 masks for 2 images"):
        ed._plan(fake_unet(TINY_CONFIG), 8, 32, 32, True)


def test_auto_editor_takes_the_reference_signature():
    ed = MutualSelfAttentionControlMaskAuto(4, 10, None, None, 50, 0.2, [1, 2], [3], None)
    assert (ed.thres, ed.ref_token_idx, ed.cur_token_idx) == (0.2, [1, 2], [3])
    d = MutualSelfAttentionControlMaskAuto()
    assert (d.start_step, d.start_layer, d.thres, d.ref_token_idx, d.cur_token_idx, d.mask_save_dir) == (4, 10, 0.1, [1], [1], None)
    with pytest.raises(ValueError, match="cur_token_idx"):
        MutualSelfAttentionControlMaskAuto(cur_token_idx=[77])
    p = MutualSelfAttentionControlMaskAuto(0, 4, ref_token_idx=[2], keep_masks=True)._plan(fake_unet(TINY_CONFIG), 4, 32, 32, True)
    assert p.masa_auto == 1 and p.masa_images == 1 and p.n_masa_rows == 2 and p.n_masa_ref == 1 and p.n_masa_res == 0
    assert p.n_masa_dump == 7 and abs(p.masa_thres - 0.1) < 1e-7               # blocks 4 .. 10 of the tiny UNet
    assert p.masa_ws_bytes == 2 * 256 * 4 + 4 * 4096 + 2 * 2 * 256 * 77 * 4


def test_mask_save_dir_writes_the_reference_file_names(tmp_path):
    from PIL import Image
    m = torch.zeros(16, 16)
    m[4:12, 4:12] = 1
    MutualSelfAttentionControlMask(0, 0, mask_s=m, mask_t=1 - m, mask_save_dir=str(tmp_path / "masks"))
    s = np.asarray(Image.open(tmp_path / "masks" / "mask_s.png"))
    t = np.asarray(Image.open(tmp_path / "masks" / "mask_t.png"))
    assert s.dtype == np.uint8 and np.array_equal(s, (m.numpy() * 255).astype(np.uint8)) and np.array_equal(t, 255 - s)


# ------------------------------------------------------------------------------------------------ plan struct, driver
def test_zero_initialised_plan_leaves_every_new_field_off():
    p = _lib.P2PPlan()
    for name in ("masa_rows", "h_masa_rows", "h_masa_cls_q", "h_masa_cls_k", "h_masa_tokens", "masa_ref_tokens", "masa_cur_tokens",
                 "masa_ws", "h_masa_dump"):
        assert not getattr(p, name), name
    for name in ("n_masa_rows", "n_masa_res", "masa_auto", "masa_images", "n_masa_ref", "n_masa_cur", "masa_ws_bytes", "n_masa_dump"):
        assert getattr(p, name) == 0, name
    assert p.masa_thres == 0.0
    names = [f[0] for f in _lib.P2PPlan._fields_]
    assert names.index("masa_rows") == names.index("n_store_self") + 1          # appended: old callers zero-fill the tail


def _driver():
    sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
    spec = importlib.util.spec_from_file_location("hedit_main_masactrl_mask", os.path.join(ROOT, "h-edit_amd", "main_masactrl.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_driver_flag_names_the_output_directory():
    from hedit import driver as DR
    m = _driver()
    today = m.build_parser().parse_args(["--step", "1", "--layer", "2"])
    assert "masa_mask" not in vars(today)
    assert m.output_tail(today) == DR.family_tail(today, "masactrl") == "_step_1_layer_2_"
    none = m.build_parser().parse_args(["--step", "1", "--layer", "2", "--masa_mask", "none"])
    assert m.output_tail(none) == "_step_1_layer_2_"
    assert isinstance(m.make_editor(none, []), MutualSelfAttentionControl) and not isinstance(m.make_editor(none, []), MutualSelfAttentionControlMask)
    pie = m.build_parser().parse_args(["--step", "1", "--layer", "2", "--masa_mask", "pie"])
    assert m.output_tail(pie) == "_step_1_layer_2__mask_pie"
    ed = m.make_editor(pie, [("k", {"mask": [512 * 100, 512 * 50]}, "a.png", "b.png"), ("k2", {}, "a.png", "b.png")])
    assert isinstance(ed, MutualSelfAttentionControlMask) and ed.mask_s.shape == (2, 512, 512) and torch.equal(ed.mask_s, ed.mask_t)
    assert ed.mask_s[0, 120, 200] == 1 and ed.mask_s[0, 300, 200] == 0 and ed.mask_s[1, 0, 5] == 1 and ed.mask_s[1, 5, 5] == 0
    with pytest.raises(SystemExit):
        m.build_parser().parse_args(["--masa_mask", "auto"])


def test_evaluator_and_driver_share_one_mask_decoder():
    from evaluation import evaluation as EV
    from hedit.pie_mask import mask_decode
    assert EV.mask_decode is mask_decode
