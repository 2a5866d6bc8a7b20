"""Host side of the Prompt-to-Prompt generation workflow and the attention viewers (hedit/p2p/ptp_utils.py: view_images,
text_under_image, diffusion_step, text2image_ldm*; hedit/p2p/ptp_classes.py: aggregate_attention, show_cross_attention;
DDIMScheduler.step; the hedit_attn_aggregate export).  No GPU: aggregate_attention runs its hook path here, on a store of plain
CPU tensors, against an fp64 restatement and against the reference's own output (tests/golden/g26_aggregate_attention.npz,
written by tests/golden/make_golden_p2p_aggregate.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import p2p_generate_ref as PR
from hedit import _lib
from hedit.p2p import ptp_classes as PC
from hedit.p2p import ptp_utils as PU
from hedit.scheduler import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 26          # the seed of the committed golden file


# ---------------------------------------------------------------------------------------------- view_images / text_under_image
def _tiles(n, h=10, w=8):
    return [np.full((h, w, 3), 10 * (i + 1), dtype=np.uint8) for i in range(n)]


def test_view_images_lays_a_row_out_with_the_offset():
    h, w = 100, 60
    tiles = _tiles(3, h, w)
    grid = np.array(PU.view_images(tiles))
    off = int(h * 0.02)
    assert off == 2 and grid.shape == (h, 3 * w + 2 * off, 3)
    for j, t in enumerate(tiles):
        assert np.array_equal(grid[:, j * (w + off):j * (w + off) + w], t)
    assert (grid[:, w:w + off] == 255).all() and (grid[:, 2 * w + off:2 * (w + off)] == 255).all()
    # a 4-d stack and a list are the same grid; one HWC image is a grid of one
    assert np.array_equal(np.array(PU.view_images(np.stack(tiles))), grid)
    assert np.array_equal(np.array(PU.view_images(tiles[0])), tiles[0])


def test_view_images_rows_and_offset_ratio():
    h, w = 50, 40
    tiles = _tiles(4, h, w)
    grid = np.array(PU.view_images(tiles, num_rows=2, offset_ratio=0.1))
    off = 5
    assert grid.shape == (2 * h + off, 2 * w + off, 3)
    for k, t in enumerate(tiles):
        i, j = divmod(k, 2)
        assert np.array_equal(grid[i * (h + off):i * (h + off) + h, j * (w + off):j * (w + off) + w], t)
    assert (grid[h:h + off] == 255).all() and (grid[:, w:w + off] == 255).all()


def test_view_images_fills_with_white_when_the_count_does_not_divide():
    h, w = 50, 40
    tiles = _tiles(3, h, w)
    grid = np.array(PU.view_images(tiles, num_rows=2))          # 3 % 2 = 1 filler: a 2 x 2 grid
    off = 1
    assert grid.shape == (2 * h + off, 2 * w + off, 3)
    assert np.array_equal(grid[h + off:, :w], tiles[2])
    assert (grid[h + off:, w + off:] == 255).all()


def test_text_under_image_canvas():
    img = np.random.default_rng(0).integers(0, 255, (100, 64, 3), dtype=np.uint8)
    out = PU.text_under_image(img, "cat")
    assert out.dtype == np.uint8 and out.shape == (100 + int(0.2 * 100), 64, 3)
    assert np.array_equal(out[:100], img)
    strip = out[100:]
    assert (strip == 255).any() and (strip != 255).any()          # white, with glyph pixels on it
    assert (PU.text_under_image(img, "")[100:] == 255).all()


# ---------------------------------------------------------------------------------------------- aggregate_attention, hook path
@pytest.fixture(scope="module")
def hook_store():
    steps = PR.fake_steps(SEED)
    store = PR.fill_store(PC.AttentionStore(), steps)
    assert store.cur_step == PR.STEPS and PC._fused_state(store) is None
    return store, steps


CASES = [(8, ("up", "down"), True), (8, ("down",), True), (4, ("down", "mid", "up"), True), (4, ("mid",), True),
         (8, ("up", "down"), False), (4, ("up",), False)]


@pytest.mark.parametrize("select", [0, 1])
@pytest.mark.parametrize("res,where,is_cross", CASES)
def test_aggregate_attention_hook_path_matches_fp64_and_the_reference(hook_store, golden_dir, res, where, is_cross, select):
    store, steps = hook_store
    got = PC.aggregate_attention(store, res, where, is_cross, select, prompts=["a", "b"])
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert tuple(got.shape) == (res, res, 77 if is_cross else res * res)
    want, abs_sum, count = PR.aggregate_ref64(steps, res, where, is_cross, select)
    bound = PR.hook_path_bound(abs_sum, count)
    err = (got.double() - want).abs()
    print(f"res {res} {where} cross={is_cross} select={select}: {count} terms, max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    other, _, _ = PR.aggregate_ref64(steps, res, where, is_cross, 1 - select)
    assert (want - other).abs().max() > 1e-3                      # the two prompts' maps are told apart
    # the reference's own function on its own store, same fake steps: the same torch operations in the same order
    g = np.load(os.path.join(golden_dir, "g26_aggregate_attention.npz"))
    ref = g[f"res{res}_{'-'.join(where)}_{'cross' if is_cross else 'self'}_{select}"]
    assert ref.shape == tuple(got.shape)
    assert (np.abs(ref.astype(np.float64) - want.numpy()) <= bound.numpy()).all()
    assert np.array_equal(got.numpy(), ref)


@pytest.mark.parametrize("res,where,is_cross", [(8, ("mid",), True), (16, ("up", "down"), True), (16, ("up", "down", "mid"), False)])
def test_aggregate_attention_names_the_resolutions_present(hook_store, res, where, is_cross):
    with pytest.raises(ValueError) as e:
        PC.aggregate_attention(hook_store[0], res, where, is_cross, 0, prompts=["a", "b"])
    assert f"{res} x {res}" in str(e.value)
    assert ("[4]" if where == ("mid",) else "[4, 8]") in str(e.value)


def test_show_cross_attention_returns_one_tile_per_token(hook_store):
    from PIL import Image
    tok = PR.StubTokenizer()
    prompts = ["a cat sat", "a dog sat"]
    assert len(tok.encode(prompts[1])) == 5
    grid = PC.show_cross_attention(hook_store[0], 8, ("up", "down"), select=1, prompts=prompts, tokenizer=tok)
    assert isinstance(grid, Image.Image)
    h = 256 + int(256 * 0.2)
    assert grid.size == (5 * 256 + 4 * int(h * 0.02), h)
    a = np.array(grid)
    # tile i is the aggregated map of token i, scaled to its maximum and resized by PIL
    maps = PC.aggregate_attention(hook_store[0], 8, ("up", "down"), True, 1, prompts)
    for i in (0, 4):
        m = maps[:, :, i]
        tile = (255 * m / m.max()).unsqueeze(-1).expand(8, 8, 3).numpy().astype(np.uint8)
        x = i * (256 + int(h * 0.02))
        assert np.array_equal(a[:256, x:x + 256], np.array(Image.fromarray(tile).resize((256, 256))))


def test_show_self_attention_comp_returns_the_grid(hook_store):
    grid = PC.show_self_attention_comp(hook_store[0], 4, ("up", "down", "mid"), max_com=3, select=0, prompts=["a", "b"])
    assert grid.size == (3 * 256, 256)


# ---------------------------------------------------------------------------------------------- refusals
def test_scheduler_step_refuses_an_unknown_timestep():
    s = DDIMScheduler()
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 1, x)
    s.set_timesteps(10)
    assert 901 in s.timesteps.tolist() and 900 not in s.timesteps.tolist()
    with pytest.raises(ValueError, match="900 is not one of the 10 timesteps"):
        s.step(x, 900, x)
    with pytest.raises(TypeError, match="float32 CUDA"):          # a known t gets as far as the kernel's operands
        s.step(x, torch.tensor(901), x)


def test_low_resource_and_the_ldm_variant_are_refused_by_name(monkeypatch):
    x = torch.zeros(2, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="low_resource"):
        PU.diffusion_step(None, PC.EmptyControl(), x, None, 1, 7.5, low_resource=True)
    with pytest.raises(NotImplementedError, match="low_resource"):
        PU.text2image_ldm_stable(None, ["a", "b"], PC.EmptyControl(), low_resource=True)
    monkeypatch.setattr(PC, "LOW_RESOURCE", True)
    with pytest.raises(NotImplementedError, match="LOW_RESOURCE"):
        PU.diffusion_step(None, PC.EmptyControl(), x, None, 1, 7.5)
    monkeypatch.setattr(PC, "LOW_RESOURCE", False)
    with pytest.raises(NotImplementedError, match="text2image_ldm"):
        PU.text2image_ldm(None, ["a", "b"], PC.EmptyControl())
    for prompt in ("one prompt", ["a"], ["a", "b", "c"]):
        with pytest.raises(NotImplementedError, match="one .source, target. prompt pair per controller"):
            PU.text2image_ldm_stable(None, prompt, PC.EmptyControl())


def test_init_latent_draws_on_the_cpu_with_the_callers_generator():
    import types
    model = types.SimpleNamespace(unet=types.SimpleNamespace(config={"in_channels": 4}), device=torch.device("cpu"))
    latent, latents = PU.init_latent(None, model, 64, 48, torch.Generator().manual_seed(5), 2)
    assert torch.equal(latent, torch.randn((1, 4, 8, 6), generator=torch.Generator().manual_seed(5)))
    assert latents.shape == (2, 4, 8, 6) and torch.equal(latents[0], latent[0]) and torch.equal(latents[1], latent[0])
    again, _ = PU.init_latent(latent, model, 64, 48, None, 2)
    assert again is latent


# ---------------------------------------------------------------------------------------------- the export
def test_attn_aggregate_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    declared = set(re.findall(r"\b(hedit_[a-z0-9_]+)\s*\(", hdr))
    assert "hedit_attn_aggregate" in declared and "hedit_attn_aggregate" in _lib.EXPORTS
    assert re.search(r"int hedit_attn_aggregate\(float\* const\* h_maps, int n_maps, int heads, int tokens, int cols, int n_img, "
                     r"int cur_step,\s+float\* out, void\* stream\);", hdr)
    for path in (_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), "libhedit_hip_f16.so")):
        assert os.path.exists(path), "build first: python h-edit_amd/build.py [--f16]"
        assert hasattr(ctypes.CDLL(path), "hedit_attn_aggregate"), path
    fn = _lib.lib().hedit_attn_aggregate
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9


def test_attn_aggregate_refuses_by_name_without_touching_a_device():
    """the argument checks come before any HIP call: on a machine with no GPU every refusal still answers by name (the
    pointers are never dereferenced)"""
    lib = _lib.lib()
    arr = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    holed = (ctypes.c_void_p * 2)(0x1000, None)
    out = ctypes.c_void_p(0x3000)
    bad = [(arr, 0, 2, 16, 77, 1, 3, out, "n_maps"), (arr, 17, 2, 16, 77, 1, 3, out, "16 maps"), (arr, 2, 2, 16, 77, 1, 0, out, "cur_step"),
           (arr, 2, 0, 16, 77, 1, 3, out, "heads"), (arr, 2, 2, 16, 0, 1, 3, out, "cols"), (arr, 2, 2, 0, 77, 1, 3, out, "tokens"),
           (arr, 2, 2, 16, 77, 0, 3, out, "n_img"), (None, 2, 2, 16, 77, 1, 3, out, "h_maps"), (arr, 2, 2, 16, 77, 1, 3, None, "out"),
           (holed, 2, 2, 16, 77, 1, 3, out, "null map")]
    for *args, what in bad:
        assert lib.hedit_attn_aggregate(*args, None) != 0, what
        assert what in lib.hedit_last_error().decode(), (what, lib.hedit_last_error().decode())
