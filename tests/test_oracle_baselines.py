"""Pin the fp32 twins of the comparison editors (tests/helpers/baseline_ref.py) on vectors produced by RUNNING the
reference's p2p_baselines / masactrl_baselines / pnp_baselines modules (tests/golden/make_golden_baselines.py, g18).
CPU only.  Limits: the ones this comparison already has -- close(..., 2e-4) of tests/test_oracle_golden.py for the toy
loops, atol 2e-4 / rtol 1e-4 of tests/test_oracle_pnp.py for the Plug-and-Play loop on the oracle SD UNet."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import baseline_ref as BR
from helpers.tiny import (PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model, make_tiny_masa_model,
                          make_tiny_model)
from oracle import masactrl as OM
from oracle import p2p as OP
from oracle import pnp as OPNP

torch.set_num_threads(4)
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GD, "g18_baselines.json")))
CASES = {c["name"]: c for c in META["cases"]}
CFG = META["cfg"]
T = 10


def vec():
    return np.load(os.path.join(GD, "g18_baselines.npz"))


def close(a, b, tol):
    a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-12
    assert err <= tol * max(1.0, ref), f"max abs err {err} (ref max {ref})"


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / b.norm())


def run_twin(case, g):
    """-> (edit, recon | None, cur_step | None)"""
    name, fam = case["name"], case["family"]
    if fam == "p2p":
        model = make_tiny_model(T)
        if case["inv"] == "ddim":
            model.scheduler = ddim_tables(T, steps_offset=0)
        pi, after = case["pair"], T - case["skip"]
        zs = torch.from_numpy(g[f"p2p_{case['inv']}{pi}_zs"])
        wts = torch.from_numpy(g[f"p2p_{case['inv']}{pi}_wts"])
        src, tar, blend, is_replace = PROMPT_PAIRS[pi]
        if not case["blend"]:
            blend = None
        if case["fn"] == "ef_wo_p2p":
            c = OP.Controller("store")
            OP.register(model, c)
            e = BR.ef_wo_p2p(model, wts[after], etas=1.0, prompts=[tar], cfg_scales=[CFG[1]], zs=zs[:after], controller=c)
            return e, None, c.cur_step
        bw = ((blend[0],), (blend[1],)) if blend else None
        eq = {"words": (blend[1],), "values": (2.0,)} if blend else None
        c = OP.make_controller([src, tar], is_replace, 0.4, 0.35, blend_word=bw, eq_params=eq, num_steps=after, tok=model.tokenizer)
        OP.register(model, c)
        e, r = BR.ef_or_pnp_inv_w_p2p(model, wts[after], etas=1.0, prompts=[src, tar], cfg_scales=CFG, zs=zs[:after], controller=c,
                                      is_ddim_inversion=case["inv"] == "ddim")
        return e, r, c.cur_step
    if fam == "masactrl":
        model = make_tiny_masa_model(T)
        ddim = case["inv"] == "ddim"
        if ddim:
            model.scheduler = ddim_tables(T, steps_offset=0)
        ed = OM.MutualSelfAttention(case["start_step"], case["start_layer"])
        OM.register_editor(model, ed)
        assert ed.num_att_layers == case["num_att_layers"]
        after = T - case["skip"]
        zs, wts = torch.from_numpy(g[f"{name}_zs"]), torch.from_numpy(g[f"{name}_wts"])
        e, r = BR.ef_or_pnp_inv_w_masactrl(model, wts[after], etas=1.0, prompts=["", PROMPT_PAIRS[0][1]], cfg_scales=CFG,
                                           zs=zs[:after], is_ddim_inversion=ddim)
        return e, r, ed.cur_step
    Tp = 4
    model, _ = make_oracle_sd_model(TINY4_CONFIG, Tp)
    model.scheduler = ddim_tables(Tp, steps_offset=0)
    OPNP.register_pnp(model, case["qk"], case["conv"])
    xT = torch.from_numpy(g["pnp_xT"])
    zs = torch.zeros(Tp, 4, 64, 64)                  # etas = 0: only its length is read
    prompts = [PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]]
    if case["fn"] == "negative_prompt_pnp":
        e, r = BR.negative_prompt_pnp(model, xT, etas=0.0, prompts=prompts, cfg_scales=CFG, zs=zs)
    else:
        e, r = BR.ef_or_pnp_inv_w_pnp(model, xT, etas=0.0, prompts=prompts, cfg_scales=CFG, zs=zs, is_ddim_inversion=True)
    return e, r, None


@pytest.mark.parametrize("name", list(CASES))
def test_twin_matches_the_reference(name):
    g, case = vec(), CASES[name]
    e, r, cur = run_twin(case, g)
    if case["family"] == "pnp":
        assert torch.allclose(e, torch.from_numpy(g[f"{name}_edit"]), atol=2e-4, rtol=1e-4)
        assert torch.allclose(r, torch.from_numpy(g[f"{name}_recon"]), atol=2e-4, rtol=1e-4)
    else:
        close(e, g[f"{name}_edit"], 2e-4)
        if case["single"]:
            # the reference's ef_wo_p2p returns ONE tensor (p2p_baselines.py:95)
            assert r is None and f"{name}_recon" not in g.files and e.shape == (1, 4, 16, 16)
        else:
            close(r, g[f"{name}_recon"], 2e-4)
        assert cur == case["cur_step"]


def test_the_cases_are_distinct_edits():
    """every case's edit is far (orders of magnitude above the 2e-4 limit) from its reconstruction, from the latent it
    started from and from every other case's edit of the same shape: a twin that hands back an input cannot pass"""
    g = vec()
    names = list(CASES)
    for n in names:
        e = g[f"{n}_edit"]
        if f"{n}_recon" in g.files:
            assert rel(e, g[f"{n}_recon"]) > 5e-2, n
        for m in names:
            if m != n and g[f"{m}_edit"].shape == e.shape:
                assert rel(e, g[f"{m}_edit"]) > 5e-2, (n, m)
    for n in ("ef_p2p_skip0", "pnp_inv_p2p"):
        assert rel(g[f"{n}_recon"], g["p2p_w0"]) < 2e-2         # the source row replays its inversion
    assert rel(g["ef_masactrl_recon"], g["masa_w0"]) < 2e-2
