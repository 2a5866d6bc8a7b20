"""No GPU: the Edit Friendly loop of the combined text + style task (hedit.inversion.ef_style.ef_p2p) on the tiny torch models
of tests/helpers/tiny.py against tests/golden/g26_ef_style.npz -- the reference's own function
(text-guided-n-style/inversion/ef.py), run unmodified by tests/golden/make_golden_ef_style.py on the same toys (10 steps;
blend word at skip 5, no blend word at skip 6, is_ddim_inversion at skip 6: the generator's docstring says why no case has
skip 0).  Both sides do the same torch-CPU arithmetic through the autograd of the same network, decoder and style encoder, so
the limits are those of tests/test_host_nmg.py: atol 5e-4, rtol 1e-4; the module runs at the generator's thread count.  The
controllers on this side are the oracle's (oracle/p2p.py), themselves pinned on the reference's.

Also here: the reference's assertions, the lock-step form, what edit_ef.py / main_edit.py run and refuse, and the two
exports of the style step's kernels."""
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.tiny import PROMPT_PAIRS, TinyStyleEncoder, TinyVae, make_tiny_model  # noqa: E402
from hedit.inversion.ef_style import ef_p2p  # noqa: E402
from oracle import p2p as OP  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def generator_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)          # make_golden_ef_style.py's
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "g26_ef_style.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "g26_ef_style.npz")), meta


def close(got, want):
    assert np.allclose(got.detach().numpy(), want, atol=5e-4, rtol=1e-4), float(np.abs(got.detach().numpy() - want).max())


def test_fixture_covers_the_cases_and_is_well_conditioned(gold):
    g, meta = gold
    cases = meta["cases"]
    assert any(c["blend"] and c["skip"] > 0 and not c["ddim"] for c in cases)
    assert any(not c["blend"] for c in cases) and any(c["ddim"] for c in cases)
    assert meta["cfg"] == [1.0, 7.5]                                        # two entries, not three
    rms0 = float(np.sqrt((g["w0"].astype(np.float64) ** 2).mean()))
    for c in cases:
        e = g[c["name"] + "_edit"].astype(np.float64)
        assert np.sqrt((e ** 2).mean()) < 3 * rms0, c["name"]


@pytest.mark.parametrize("ci", range(3))
def test_ef_p2p_matches_the_reference(gold, ci):
    g, meta = gold
    case = meta["cases"][ci]
    T, pi = meta["T"], case["pair"]
    model = make_tiny_model(T)
    model.vae = TinyVae()
    after = T - case["skip"]
    zs, wts = torch.from_numpy(g[case["name"] + "_zs"]), torch.from_numpy(g[case["name"] + "_wts"])
    src, tar, blend, is_replace = PROMPT_PAIRS[pi]
    if not case["blend"]:
        blend = None
    ctrl = OP.make_controller([src, tar], is_replace, 0.4, 0.35, blend_word=((blend[0],), (blend[1],)) if blend else None,
                              eq_params={"words": (blend[1],), "values": (2.0,)} if blend else None, num_steps=after,
                              tok=model.tokenizer)
    OP.register(model, ctrl)
    edit, recon = ef_p2p(model, TinyStyleEncoder(), xT=wts[after], etas=1.0, prompts=[src, tar], cfg_scales=meta["cfg"],
                         zs=zs[:after], controller=ctrl, weight_edit_clip=case["weight"], is_ddim_inversion=case["ddim"])
    assert edit.shape == recon.shape == (1, 4, 16, 16)
    assert ctrl.cur_step == case["cur_step"] == after       # one controlled pass per step: the gradient pass does not count
    close(edit, g[case["name"] + "_edit"])
    close(recon, g[case["name"] + "_recon"])


def test_target_row_steps_with_eta_0_under_ddim_inversion(gold):
    """the reference's quirk (ef.py:86-87): with is_ddim_inversion the target row ignores the noise map, the source row adds
    eta * z -- so another z moves the reconstruction and leaves the edit where it was (no local blend: the rows do not mix)"""
    g, meta = gold
    T, after = meta["T"], 3
    name = meta["cases"][0]["name"]
    zs, wts = torch.from_numpy(g[name + "_zs"]), torch.from_numpy(g[name + "_wts"])

    def run(z, ddim):
        model = make_tiny_model(T)
        model.vae = TinyVae()
        return ef_p2p(model, TinyStyleEncoder(), xT=wts[after], etas=1.0, prompts=list(PROMPT_PAIRS[2][:2]), cfg_scales=meta["cfg"],
                      zs=z, controller=None, weight_edit_clip=0.5, is_ddim_inversion=ddim)

    a, b = run(zs[:after], True), run(zs[:after] * 0.5, True)
    assert torch.equal(a[0], b[0]) and not torch.allclose(a[1], b[1], atol=1e-3)
    c, d = run(zs[:after], False), run(zs[:after] * 0.5, False)
    assert not torch.allclose(c[0], d[0], atol=1e-3)


class ElementwiseUNet:
    """a differentiable eps-model whose rows cannot see each other and whose arithmetic is elementwise, so a row of a batch has
    the bits of the same row alone (a matrix product on the CPU promises no such thing)"""

    def __call__(self, x, t, encoder_hidden_states=None, cross_attention_kwargs=None):
        c = encoder_hidden_states.mean(dim=(1, 2)).view(-1, 1, 1, 1)
        return types.SimpleNamespace(sample=torch.tanh(1.3 * x + 5.0 * c) * 0.7 + 0.05 * x * x * math.cos(float(t)))


def test_lock_step_equals_the_single_runs(gold):
    """two images with per_image=True, each with its own prompts, noise maps and style encoder == the two single runs, bit for
    bit over four steps: the eps-model is elementwise (see ElementwiseUNet) and the loop decodes and scores image by image.  On
    the GPU the library is batch-invariant and the driver test compares whole runs byte for byte."""
    g, meta = gold
    T, after = meta["T"], 4
    names = [meta["cases"][0]["name"], meta["cases"][1]["name"]]
    wts = torch.stack([torch.from_numpy(g[n + "_wts"]) for n in names], dim=1)       # (T + 1, 2, C, H, W)
    zs = torch.stack([torch.from_numpy(g[n + "_zs"]) for n in names], dim=1)
    pairs = [list(PROMPT_PAIRS[2][:2]), list(PROMPT_PAIRS[0][:2])]
    encs = [TinyStyleEncoder(), TinyStyleEncoder(seed=77)]

    def run(sel):
        model = make_tiny_model(T)
        model.unet = ElementwiseUNet()
        model.vae = TinyVae()
        model.text_encoder = lambda ids: (torch.sin(ids.float()).unsqueeze(-1).expand(-1, -1, 8),)      # a lookup: no matrix product
        # the toy tokenizer numbers words in the order it meets them: the same order in every run
        model.tokenizer([w for pr in pairs for w in pr], padding="max_length", max_length=model.tokenizer.model_max_length,
                        truncation=True, return_tensors="pt")
        one = len(sel) == 1
        return ef_p2p(model, encs[sel[0]] if one else [encs[j] for j in sel], xT=wts[after][sel], etas=1.0,
                      prompts=pairs[sel[0]] if one else [pairs[j] for j in sel], cfg_scales=meta["cfg"], zs=zs[:after][:, sel],
                      controller=None, weight_edit_clip=0.8, per_image=True)

    both = run([0, 1])
    assert both[0].shape == (2, 4, 16, 16)
    for j in (0, 1):
        one = run([j])
        for b, o in zip(both, one):
            assert torch.isfinite(o).all() and torch.equal(b[j:j + 1], o), j
    assert not torch.allclose(both[0][0], both[0][1], atol=1e-3)
    with pytest.raises(ValueError):          # pairs of prompts without per_image: not the reference's call
        ef_p2p(make_tiny_model(T), encs, xT=wts[after], prompts=pairs, cfg_scales=meta["cfg"], zs=zs[:after])


def test_reference_assertions_are_kept():
    model = types.SimpleNamespace(scheduler=types.SimpleNamespace(num_inference_steps=4))
    with pytest.raises(AssertionError):                   # two prompts (ef.py:39)
        ef_p2p(model, None, None, prompts=["a"], cfg_scales=[1.0, 7.5])
    with pytest.raises(AssertionError):                   # one eta per inference step (ef.py:49)
        ef_p2p(model, None, None, etas=[1.0] * 3, prompts=["a", "b"], cfg_scales=[1.0, 7.5])


def test_fused_step_is_refused_off_the_hip_unet(gold):
    from hedit.inversion.ef_style import ef_style_update
    model = make_tiny_model(4)
    with pytest.raises(RuntimeError) as ei:
        ef_style_update(model, None, None, None, None, None, 1, 7.5, 1.5, fused=True)
    assert "HIP" in str(ei.value)


def _driver(name):
    spec = importlib.util.spec_from_file_location("hedit_" + name, os.path.join(ROOT, "h-edit_amd", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_driver_defaults_to_ef_p2p_and_refuses_other_modes(monkeypatch):
    d = _driver("edit_ef")
    seen = {}
    monkeypatch.setattr(d.main_edit, "main", lambda argv, modes: seen.update(args=d.main_edit.build_parser().parse_args(argv), modes=modes))
    d.main(["--skip", "2"])
    assert seen["args"].mode == "ef_p2p" and seen["modes"] == ("ef_p2p",) and seen["args"].skip == 2
    assert seen["args"].weight_edit_clip_for_ef == 1.5 and seen["args"].weight_edit_clip == 0.5
    monkeypatch.undo()
    for mode in ("h_edit_R_p2p", "ef", "nmg_p2p"):
        with pytest.raises(NotImplementedError) as ei:
            d.main(["--mode", mode])
        assert mode in str(ei.value) and "ef_p2p" in str(ei.value)
    for flags in (["--eta", "0.5"], ["--optimization_steps", "2"]):          # the reference's assertions (main_edit.py:76-78)
        with pytest.raises(AssertionError):
            d.main(flags)
    assert "w_style_" in d.__doc__ and "weight_edit_clip_for_ef" in d.__doc__       # the folder name's quirk is documented


def test_main_edit_still_refuses_ef_p2p():
    d = _driver("main_edit")
    with pytest.raises(NotImplementedError) as ei:
        d.main(["--mode", "ef_p2p"])
    assert "ef_p2p" in str(ei.value) and "edit_ef.py" in str(ei.value)
    with pytest.raises(NotImplementedError):
        d.main(["--mode", "h_edit_R_p2p"], modes=("ef_p2p",))
    assert vars(d.build_parser().parse_args([]))["mode"] == "h_edit_R_p2p"


def test_the_step_kernels_are_declared_and_exported():
    from hedit import _lib
    header = open(os.path.join(ROOT, "include", "hedit.h")).read()
    for n in ("hedit_step_ef_seed", "hedit_step_ef_style"):
        assert f"int {n}(" in header and n in _lib.EXPORTS, n
        assert header.count(n) >= 2, n                      # the declaration and the call-site table
