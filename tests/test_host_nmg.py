"""No GPU: the Noise Map Guidance loops of hedit.inversion (nmg_p2p, nmg_pnp) on the tiny torch models of
tests/helpers/tiny.py against tests/golden/g22_nmg.npz -- the reference's own functions, run unmodified by
tests/golden/make_golden_nmg.py on the same toys (10 steps, skip 0 and 3, with and without blend words; nmg_pnp on the
four-level toy at 4 steps).  Both sides do the same torch-CPU arithmetic through the autograd of the same network, so the
limits are those of tests/test_host_face_ef.py against g21_face_ef.npz: atol 5e-4, rtol 1e-4.  The controllers and the
injection hooks on this side are the oracle's (oracle/p2p.py, oracle/pnp.py), themselves pinned on the reference's.

"The same arithmetic" is meant literally.  The guidance term is sign(residual) / numel times grad_scale * guidance_noise_map =
5e4, on random weights a map that turns a last-bit difference into an O(1) one within ten steps (the reconstruction row
reaches 1e3): measured here, hedit's loops give the reference's BITS with the reference's or the oracle's processors at 1
and at 4 threads, and 16 threads (another summation order inside the matrix products) move the 10-step result by 3.7 of
22.  So the module runs at the generator's thread count.

Also here: the reference's assertions, the per-image L1 mean of the lock-step form, and what main_nmg.py / main_baselines.py
run and refuse."""
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
from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model, make_tiny_model  # noqa: E402
from hedit.inversion.p2p_baselines import nmg_p2p  # noqa: E402
from hedit.inversion.pnp_baselines import nmg_pnp  # noqa: E402
from oracle import p2p as OP  # noqa: E402
from oracle import pnp as ON  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def generator_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)          # make_golden_nmg.py's
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "g22_nmg.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "g22_nmg.npz")), meta


def close(got, want):
    assert np.allclose(got.detach().numpy(), want, atol=5e-4, rtol=1e-4), float(np.abs(got.detach().numpy() - want).max())


def tiny_ddim(T):
    model = make_tiny_model(T)
    model.scheduler = ddim_tables(T, steps_offset=0)
    return model


def controller_for(model, case, after):
    if not case["p2p"]:
        return OP.Controller("store")
    pair = PROMPT_PAIRS[case["pair"]]
    if not case["blend"]:
        pair = pair[:2] + (None, pair[3])
    src, tar, blend, is_replace = pair
    bw = ((blend[0],), (blend[1],)) if blend else None
    eq = {"words": (blend[1],), "values": (2.0,)} if blend else None
    return OP.make_controller([src, tar], is_replace, 0.4, 0.35, blend_word=bw, eq_params=eq, num_steps=after, tok=model.tokenizer)


@pytest.mark.parametrize("ci", range(4))
def test_nmg_p2p_matches_the_reference(gold, ci):
    g, meta = gold
    case = [c for c in meta["cases"] if c["family"] == "p2p"][ci]
    T, pi = meta["T"], case["pair"]
    model = tiny_ddim(T)
    after = T - case["skip"]
    zs, wts = torch.from_numpy(g[f"p2p_inv{pi}_zs"]), torch.from_numpy(g[f"p2p_inv{pi}_wts"])
    ctrl = controller_for(model, case, after)
    OP.register(model, ctrl)
    edit, recon = nmg_p2p(model, xT=wts[after], xT_ori=wts[:after + 1], etas=0.0, prompts=list(PROMPT_PAIRS[pi][:2]),
                          cfg_scales=meta["cfg"], zs=zs[:after], controller=ctrl, **meta["nmg"])
    assert edit.shape == recon.shape == (1, 4, 16, 16)
    assert ctrl.cur_step == case["cur_step"]
    close(edit, g[case["name"] + "_edit"])
    close(recon, g[case["name"] + "_recon"])


def test_nmg_pnp_matches_the_reference(gold):
    g, meta = gold
    case = [c for c in meta["cases"] if c["family"] == "pnp"][0]
    T = meta["T_pnp"]
    model, _ = make_oracle_sd_model(TINY4_CONFIG, T)
    model.scheduler = ddim_tables(T, steps_offset=0)
    ON.register_pnp(model, case["qk"], case["conv"])
    wts = torch.from_numpy(g["pnp_wts"])
    edit, recon = nmg_pnp(model, xT=wts[T], xT_ori=wts[:T + 1], etas=0.0, prompts=list(PROMPT_PAIRS[0][:2]), cfg_scales=meta["cfg"],
                          zs=torch.zeros(T, 1), register_time=ON.register_time, **meta["nmg"])
    close(edit, g["nmg_pnp_edit"])
    close(recon, g["nmg_pnp_recon"])


class ElementwiseUNet:
    """a differentiable eps-model whose rows cannot see each other and whose arithmetic is elementwise, so a row of a batch has
    the bits of the same row alone (a matrix product on the CPU promises no such thing)"""

    def __call__(self, x, t, encoder_hidden_states=None, cross_attention_kwargs=None):
        c = encoder_hidden_states.mean(dim=(1, 2)).view(-1, 1, 1, 1)
        return types.SimpleNamespace(sample=torch.tanh(1.3 * x + 5.0 * c) * 0.7 + 0.05 * x * x * math.cos(float(t)))


def test_lock_step_takes_the_l1_mean_per_image(gold):
    """Entry j of a per_image batch is its single run, bit for bit, over four steps; the reference's mean over the batch
    would halve every gradient.  On an elementwise eps-model: with the tiny UNet a two-row matrix product need not have the
    bits of a one-row one on the CPU, and the loop turns a last-bit difference into an O(1) one within two steps (module
    docstring).  On the GPU the library is batch-invariant and the driver test compares whole runs byte for byte."""
    g, meta = gold
    T, after = meta["T"], 4
    wts = torch.cat([torch.from_numpy(g["p2p_inv0_wts"]), torch.from_numpy(g["p2p_inv2_wts"])], dim=1)       # (T + 1, 2, C, H, W)
    pairs = [list(PROMPT_PAIRS[0][:2]), list(PROMPT_PAIRS[2][:2])]
    kw = dict(etas=0.0, cfg_scales=meta["cfg"], zs=torch.zeros(after, 1), **meta["nmg"])

    def run(sel, per_image):
        model = tiny_ddim(T)
        model.unet = ElementwiseUNet()
        model.text_encoder = lambda ids: (torch.sin(ids.float()).unsqueeze(-1).expand(-1, -1, 8),)      # a lookup: no matrix product either
        # the toy tokenizer numbers words in the order it meets them: the same order in every run
        model.tokenizer([w for pr in pairs for w in pr], padding="max_length", max_length=model.tokenizer.model_max_length,
                        truncation=True, return_tensors="pt")
        p = [pairs[j] for j in sel]
        return nmg_p2p(model, xT=wts[after][sel], xT_ori=wts[:after + 1][:, sel], prompts=p if len(p) > 1 else p[0], controller=None,
                       per_image=per_image, **kw)

    both = run([0, 1], True)
    for j in (0, 1):
        one = run([j], True)
        plain = run([j], False)
        for b, o, q in zip(both, one, plain):
            assert torch.isfinite(o).all() and torch.equal(b[j:j + 1], o), j
            assert torch.equal(o, q)                         # one image: the per-image mean IS the reference's
    mean = run([0, 1], False)
    assert not torch.allclose(mean[1], both[1], atol=1e-3)   # the batch mean is another (weaker) guidance


def test_reference_assertions_are_kept():
    model = types.SimpleNamespace(scheduler=types.SimpleNamespace(num_inference_steps=4))
    for fn in (nmg_p2p, nmg_pnp):
        with pytest.raises(AssertionError):                   # etas must be 0 (p2p_baselines.py:222, pnp_baselines.py:59)
            fn(model, None, None, etas=1.0, prompts=["a", "b"], cfg_scales=[1.0, 7.5])
        with pytest.raises(AssertionError):                   # two prompts
            fn(model, None, None, etas=0, prompts=["a"], cfg_scales=[1.0, 7.5])


def _driver(name):
    spec = importlib.util.spec_from_file_location("hedit_" + name, os.path.join(ROOT, "h-edit_amd", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_driver_modes_and_refusals():
    d = _driver("main_nmg")
    assert d.MODES == {"nmg": "p2p", "nmg_p2p": "p2p", "nmg_pnp": "pnp"}
    with pytest.raises(NotImplementedError) as ei:
        d.main(["--mode", "nt_pnp"])
    assert "nt_pnp" in str(ei.value) and "context" in str(ei.value)
    with pytest.raises(NotImplementedError) as ei:
        d.main(["--mode", "ef_p2p"])
    assert "main_baselines.py" in str(ei.value)
    for mode in d.MODES:
        with pytest.raises(AssertionError):                   # NMG is deterministic: the DDIM inversion, eta = 0
            d.main(["--mode", mode, "--eta", "1.0"])
    assert "dispatch" in d.__doc__ and "nmg_p2p" in d.__doc__     # the deliberate difference is documented


@pytest.mark.parametrize("mode", ["nmg", "nmg_p2p", "nmg_pnp"])
def test_main_baselines_still_refuses_the_nmg_modes(mode):
    with pytest.raises(NotImplementedError) as ei:
        _driver("main_baselines").main(["--mode", mode])
    assert mode in str(ei.value) and "gradient" in str(ei.value) and "main_nmg.py" in str(ei.value)
