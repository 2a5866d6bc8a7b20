"""-m gpu: the gradient-free comparison editors (Edit Friendly, PnP Inversion, negative-prompt inversion) on the HIP
path -- hedit_step_pair, HEditEngine.run_direct / run_direct_pnp, the reference-signature functions of
hedit.inversion.{p2p,masactrl,pnp}_baselines and the main_baselines.py driver -- against the reference's vectors (g2,
g18) and the fp32 twins pinned on them (tests/helpers/baseline_ref.py, tests/test_oracle_baselines.py).

Tolerances of group 3 (relative L2 of the final latents, HIP path vs the fp32 twin on the same synthetic network and the
same inversion outputs; MEASURED on MI355X, limits = 2x the largest figure of a group, the convention of
tests/test_gpu_loops.py:15-22):
                                       chain   bf16 edit   bf16 recon   f16 edit   f16 recon
  ef_wo_p2p           pair 0, skip 3     5     2.51e-2        -         2.98e-3       -
  ef_p2p (blend)      pair 0, skip 4     4     2.03e-2     3.00e-3      2.50e-3    3.78e-4
  ef_p2p (no blend)   pair 2, skip 3     5     2.39e-2     4.25e-3      3.06e-3    5.51e-4
  pnp_inv_p2p         pair 0, skip 4     4     1.60e-2     2.44e-3      2.06e-3    2.92e-4
  ef_masactrl         skip 4             4     2.01e-2     3.16e-3      2.48e-3    3.83e-4
  pnp_inv_masactrl    skip 3             5     2.07e-2     3.47e-3      2.51e-3    4.35e-4
  ef_p2p (blend)      pair 0, skip 0     8     3.28e-2     2.08e-2      4.07e-3    2.59e-3
  np_pnp              four-level, 64x64  4     6.18e-2     9.91e-3      7.88e-3    1.27e-3
  pnp_inv_pnp, eta 0  four-level, 64x64  4     3.62e-2     9.91e-3      4.61e-3    1.27e-3
Groups and limits (edit, recon), bfloat16; half storage takes a quarter of them (helpers.gpu.lim) and measures an eighth:
  chain5  (4- and 5-step chains, TINY_CONFIG, T = 8)   5.0e-2, 8.5e-3     [test_gpu_loops.tol: 7e-2, 1.5e-2]
  chain8  (the full 8-step chain)                      6.6e-2, 4.2e-2     [test_gpu_loops.tol: 1e-1, 4.2e-2]
  pnp_inv_pnp (four-level network, T = 4)              7.3e-2, 2.0e-2     [tests/test_gpu_pnp.py, same network: 8e-2, 3e-2]
  np_pnp      (the same)                               1.24e-1, 2.0e-2
Applying cfg_tar = 7.5 to the whole eps did NOT cost accuracy on the 4 / 5 / 8-step chains: every figure is below the
h-Edit loops' on the same network.  The one limit above test_gpu_loops.tol is np_pnp's edit: the figure itself (6.2e-2) is
under 7e-2, its doubling is not.  Two terms carry it.  (a) The network and the schedule, not the method: the Plug-and-Play
cases need the four-level layout at 64 x 64 and run T = 4, 250-timestep jumps; the h-Edit loop on that network has 8e-2.
(b) Negative-prompt inversion guides BOTH rows with cfg_tar from the source embedding: under one identical bf16 rounding
of every UNet output the fp32 twin of np_pnp moves 1.84x as far as that of ef_or_pnp_inv_w_pnp (8.6e-3 vs 4.7e-3 edit;
h_edit_pnp_implicit 7.1e-3: tests/diag/diag_baselines_rounding.py) -- on the GPU the ratio is 1.71.  Both scale with the
storage format's mantissa (f16 / bf16 = 1 / 7.8), i.e. they are rounding, not arithmetic.
GPU time of this file on MI355X (pytest --durations=0, summed over its 37 tests): 11.6 s in bfloat16 (14 s wall), 11.0 s in
half storage -- of the 45 s it may take.
"""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from helpers import baseline_ref as BR  # noqa: E402
from helpers import gpu as G  # noqa: E402
from helpers.datasets import pie_dataset as _dataset  # noqa: E402
from helpers.models import make_pair  # noqa: E402
from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.unet import TINY_CONFIG  # noqa: E402

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 8
CFG = [1.0, 7.5]


# ------------------------------------------------------------------------------------------ 1, 2: the kernel
def _pair(lib, e_u, e_c, xt, z, n, kinds, coefs):
    out = torch.zeros_like(xt)
    arr = (_lib.StepCoef * kinds)(*coefs)
    _lib.check(lib.hedit_step_pair(_lib.ptr(e_u), _lib.ptr(e_c), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out), n, xt[0, 0].numel(),
                                   kinds, arr, None))
    G.sync()
    return out


def test_step_pair_matches_the_reference_reverse_step():
    """hedit_step_pair against the reference's reverse_step outputs (g2): e_u = e_c = eps, every (t, eta, ddim) of the
    fixture, the two kinds given DIFFERENT coefficient sets in one call.  fp32 arithmetic: hedit_step_base's limit on the
    same fixture (tests/test_gpu_kernels.py:604)."""
    from hedit.engine import Schedule
    lib = _lib.lib()
    g = np.load(os.path.join(GD, "g2_reverse_step.npz"))
    S = Schedule(ddim_tables(20))
    eps, x, z = (torch.from_numpy(g[k]) for k in ("eps", "x", "z"))
    combos = [(t, eta, ddim) for t in (951, 501, 1) for eta in (0.0, 1.0) for ddim in (False, True)]
    ed, xd, zd = G.f32(eps[:, None]), G.f32(x[:, None]), G.f32(z[None])          # [kind][1 image][C,H,W]
    for i, a in enumerate(combos):
        b = combos[(i + 5) % len(combos)]
        coefs = [S.step_coef(t, 0, eta, ddim, (w, 0.0, 0.0), coeff=0.0) for (t, eta, ddim), w in ((a, 1.0), (b, 7.5))]
        out = _pair(lib, ed, ed, xd, zd, 1, 2, coefs)
        for k, (t, eta, ddim) in enumerate((a, b)):
            want = torch.from_numpy(g[f"prev_t{t}_eta{int(eta)}_ddim{int(ddim)}"])[k]
            err = G.max_err(out[k, 0], want)
            print("step_pair g2", k, t, eta, ddim, err)
            assert err < 2e-5 * max(1.0, want.abs().max().item())
        one = _pair(lib, ed[1:], ed[1:], xd[1:], zd, 1, 1, coefs[1:])                 # n_kinds = 1: the same row alone
        assert torch.equal(one[0], out[1])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("with_z", [True, False])
@pytest.mark.parametrize("elems", [4 * 32 * 32, 3 * 7 * 5])
def test_step_pair_equals_step_base_on_equal_coefficients(n, with_z, elems):
    """both kinds on ONE coefficient set: the bits of hedit_step_base(rows = 4) (the vector path and, with an element count
    that is not a multiple of four, the scalar one)"""
    from hedit.engine import Schedule
    lib = _lib.lib()
    S = Schedule(ddim_tables(20))
    g = torch.Generator().manual_seed(17 * n + elems)
    e = G.f32(torch.randn(4, n, elems, generator=g))
    xt = G.f32(torch.randn(2, n, elems, generator=g))
    z = G.f32(torch.randn(n, elems, generator=g)) if with_z else None
    for t, eta, ddim, w in ((501, 1.0, False, 1.0), (951, 1.0, True, 7.5), (1, 0.0, False, 3.0)):
        coef = S.step_coef(t, 0, eta, ddim, (w, 0.0, 0.0), coeff=0.0)
        base = torch.zeros_like(xt)
        _lib.check(lib.hedit_step_base(_lib.ptr(e), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(base), n, elems, 4, C.byref(coef), None))
        pair = _pair(lib, e[:2], e[2:], xt, z, n, 2, [coef, coef])
        assert torch.equal(pair, base)
        assert torch.isfinite(pair).all() and pair.abs().max() > 0


# ------------------------------------------------------------------------------------------ 3: wrappers vs the twin
@pytest.fixture(scope="module")
def setup():
    from oracle import loops as OL
    hip, om, _ = make_pair(TINY_CONFIG, T, out_scale=0.3)
    torch.manual_seed(11)
    w0 = torch.randn(1, 4, 32, 32) * 0.8
    inv = {}
    for key, prompt in ((0, PROMPT_PAIRS[0][0]), (2, PROMPT_PAIRS[2][0]), ("", "")):
        torch.manual_seed(100 + (key or 0))
        zs, wts, _ = OL.ddpm_inversion(om, w0, eta=1.0, prompt=prompt, cfg_src=1.0, T=T)
        inv["ddpm", key] = (zs, wts)
    return hip, om, w0, inv


def _ddim(setup, prompt):
    """the eta = 0 scheduler (steps_offset 0) on both models and the oracle's DDIM inversion; undone by _ddpm"""
    from oracle import loops as OL
    from hedit.scheduler import DDIMScheduler
    hip, om, w0, inv = setup
    for m in (hip, om):
        m.scheduler = DDIMScheduler(steps_offset=0)
        m.scheduler.set_timesteps(T)
    if ("ddim", prompt) not in inv:
        from oracle.sd_unet import PlainProcessor
        om.unet.set_attn_processor({k: PlainProcessor() for k in om.unet.attn_processors})      # (an earlier test's controller)
        _, zs, lats = OL.ddim_inversion(om, w0, prompt, 1.0)
        inv["ddim", prompt] = (zs, torch.stack([l[0] for l in lats]))
    return inv["ddim", prompt]


def _ddpm(setup):
    from hedit.scheduler import DDIMScheduler
    for m in setup[:2]:
        m.scheduler = DDIMScheduler()
        m.scheduler.set_timesteps(T)


def _p2p_controllers(hip, om, pi, after, blend=True):
    from oracle import p2p as OP
    from hedit.p2p import ptp_controller_utils as PCU
    from hedit.p2p.ptp_utils import register_attention_control
    src, tar, bl, is_replace = PROMPT_PAIRS[pi]
    bl = bl if blend else None
    bw = ((bl[0],), (bl[1],)) if bl else None
    eq = {"words": (bl[1],), "values": (2.0,)} if bl else None
    hc = PCU.make_controller([src, tar], is_replace, 0.4, 0.35, blend_word=bw, equilizer_params=eq, num_steps=after,
                             tokenizer=hip.tokenizer, device=hip.device)
    oc = OP.make_controller([src, tar], is_replace, 0.4, 0.35, blend_word=bw, eq_params=eq, num_steps=after, tok=om.tokenizer)
    register_attention_control(hip, hc)
    OP.register(om, oc)
    return hc, oc


# limits: 2x the largest measured figure of the group (table in the header); (edit, recon)
TOL = {"chain5": (5.0e-2, 8.5e-3), "chain8": (6.6e-2, 4.2e-2), "pnp_inv_pnp": (7.3e-2, 2.0e-2), "np_pnp": (1.24e-1, 2.0e-2)}


def _check(name, group, e_h, e_o, r_h=None, r_o=None):
    fe = G.rel_err(e_h, e_o)
    fr = G.rel_err(r_h, r_o) if r_h is not None else float("nan")
    print(f"baseline-figure {_lib.STORAGE} {name} group={group} edit={fe:.3e} recon={fr:.3e}")
    assert torch.isfinite(e_h).all()
    G.within(fe, TOL[group][0], what=name + " edit")
    if r_h is not None:
        G.within(fr, TOL[group][1], what=name + " recon")


def test_ef_wo_p2p_matches_the_twin(setup):
    from oracle import p2p as OP
    from hedit.inversion.p2p_baselines import ef_wo_p2p
    from hedit.p2p import ptp_classes as PC
    from hedit.p2p.ptp_utils import register_attention_control
    hip, om, w0, inv = setup
    zs, wts = inv["ddpm", 0]
    after = T - 3
    hc, oc = PC.AttentionStore(), OP.Controller("store")
    register_attention_control(hip, hc)
    OP.register(om, oc)
    tar = PROMPT_PAIRS[0][1]
    e_o = BR.ef_wo_p2p(om, wts[after], etas=1.0, prompts=[tar], cfg_scales=[7.5], zs=zs[:after], controller=oc)
    e_h = ef_wo_p2p(hip, xT=G.f32(wts[after]), etas=1.0, prompts=[tar], cfg_scales=[7.5], prog_bar=False, zs=G.f32(zs[:after]),
                    controller=hc)
    G.sync()
    assert isinstance(e_h, torch.Tensor) and e_h.shape == (1, 4, 32, 32)        # ONE tensor, as the reference returns
    assert hc.cur_step == oc.cur_step == 0
    _check("ef skip3", "chain5", e_h, e_o)


@pytest.mark.parametrize("pi,skip,blend,ddim", [(0, 4, True, False), (2, 3, False, False), (0, 0, True, False), (0, 4, True, True)])
def test_ef_or_pnp_inv_w_p2p_matches_the_twin(setup, pi, skip, blend, ddim):
    from hedit.inversion.p2p_baselines import ef_or_pnp_inv_w_p2p
    hip, om, w0, inv = setup
    src, tar = PROMPT_PAIRS[pi][:2]
    after = T - skip
    try:
        zs, wts = _ddim(setup, src) if ddim else inv["ddpm", pi]
        hc, oc = _p2p_controllers(hip, om, pi, after, blend)
        kw = dict(etas=1.0, prompts=[src, tar], cfg_scales=CFG, is_ddim_inversion=ddim)
        e_o, r_o = BR.ef_or_pnp_inv_w_p2p(om, wts[after], zs=zs[:after], controller=oc, **kw)
        e_h, r_h = ef_or_pnp_inv_w_p2p(hip, xT=G.f32(wts[after]), zs=G.f32(zs[:after]), controller=hc, prog_bar=False, **kw)
        G.sync()
    finally:
        _ddpm(setup)
    assert e_h.shape == (1, 4, 32, 32) and r_h.shape == (1, 4, 32, 32)
    assert hc.cur_step == oc.cur_step == after
    _check(f"{'pnp_inv' if ddim else 'ef'}_p2p pair{pi} skip{skip} blend{int(blend)}", "chain5" if after <= 5 else "chain8", e_h, e_o, r_h, r_o)
    # the source row replays its inversion: the tol_recon tests/test_gpu_loops.py:21-22,113 applies to this invariant
    G.within(G.rel_err(r_h, w0), 1.5e-2 if after <= 5 else 4.2e-2, what="recon returns w0")


@pytest.mark.parametrize("skip,step,layer,ddim", [(4, 1, 2, False), (3, 0, 0, True)])
def test_ef_or_pnp_inv_w_masactrl_matches_the_twin(setup, skip, step, layer, ddim):
    from oracle import masactrl as OM
    from hedit.inversion.masactrl_baselines import ef_or_pnp_inv_w_masactrl
    from hedit.masactrl import MutualSelfAttentionControl, regiter_attention_editor_diffusers
    hip, om, w0, inv = setup
    after = T - skip
    tar = PROMPT_PAIRS[0][1]
    try:
        zs, wts = _ddim(setup, "") if ddim else inv["ddpm", ""]
        ed_h, ed_o = MutualSelfAttentionControl(step, layer), OM.MutualSelfAttention(step, layer)
        regiter_attention_editor_diffusers(hip, ed_h)
        OM.register_editor(om, ed_o)
        kw = dict(etas=1.0, prompts=["", tar], cfg_scales=CFG, is_ddim_inversion=ddim)
        e_o, r_o = BR.ef_or_pnp_inv_w_masactrl(om, wts[after], zs=zs[:after], **kw)
        e_h, r_h = ef_or_pnp_inv_w_masactrl(hip, xT=G.f32(wts[after]), zs=G.f32(zs[:after]), prog_bar=False, **kw)
        G.sync()
    finally:
        _ddpm(setup)
        from hedit.unet import AttnProcessor
        from oracle.sd_unet import PlainProcessor
        hip.unet._attention_editor = None
        om.unet.set_attn_processor({k: PlainProcessor() for k in om.unet.attn_processors})
        hip.unet.set_attn_processor({k: AttnProcessor() for k in hip.unet.attn_processors})
    assert ed_h.cur_step == ed_o.cur_step == after
    _check(f"{'pnp_inv' if ddim else 'ef'}_masactrl skip{skip}", "chain5", e_h, e_o, r_h, r_o)


@pytest.mark.parametrize("name", ["np_pnp", "pnp_inv_pnp_eta0"])
def test_pnp_baselines_match_the_reference_vectors(name):
    """Plug-and-Play needs the four-level layout: as tests/test_gpu_pnp.py, the HIP path on make_pair(TINY4_CONFIG) against
    the vectors of the REFERENCE's own loop on the same network (g18), on which the twin is pinned to 2e-4."""
    from hedit.inversion import pnp_baselines as PB
    from hedit.plug_n_play import register_attention_control_efficient, register_conv_control_efficient
    from hedit.scheduler import DDIMScheduler
    case = {c["name"]: c for c in json.load(open(os.path.join(GD, "g18_baselines.json")))["cases"]}[name]
    vec = np.load(os.path.join(GD, "g18_baselines.npz"))
    Tp = 4
    hip, _, _ = make_pair(TINY4_CONFIG, Tp, out_scale=0.3)
    hip.scheduler = DDIMScheduler(steps_offset=0)
    hip.scheduler.set_timesteps(Tp)
    register_attention_control_efficient(hip, case["qk"])
    register_conv_control_efficient(hip, case["conv"])
    xT, zs = G.f32(torch.from_numpy(vec["pnp_xT"])), torch.zeros(Tp, 4, 64, 64, device=G.dev())
    prompts = [PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]]
    if name == "np_pnp":
        e, r = PB.negative_prompt_pnp(hip, xT, etas=0.0, prompts=prompts, cfg_scales=CFG, prog_bar=False, zs=zs)
    else:
        e, r = PB.ef_or_pnp_inv_w_pnp(hip, xT, etas=0.0, prompts=prompts, cfg_scales=CFG, prog_bar=False, zs=zs, is_ddim_inversion=True)
        with pytest.raises(AssertionError):        # the reference's assertion (pnp_baselines.py:338), kept
            PB.ef_or_pnp_inv_w_pnp(hip, xT, etas=1.0, prompts=prompts, cfg_scales=CFG, zs=zs)
    G.sync()
    assert e.shape == (1, 4, 64, 64)
    _check(name, "np_pnp" if name == "np_pnp" else "pnp_inv_pnp", e, torch.from_numpy(vec[f"{name}_edit"]), r, torch.from_numpy(vec[f"{name}_recon"]))


# ------------------------------------------------------------------------------------------ 4, 5: bit-level properties
@pytest.fixture(scope="module")
def full_gain():
    return make_pair(TINY_CONFIG, 10)[0]


def _images(n, seed, S=32):
    return torch.stack([torch.randn(4, S, S, generator=torch.Generator().manual_seed(seed + i)) * 0.8 for i in range(n)]).to(G.dev())


def _batch_controller(hip, pis, num_steps):
    from hedit.p2p import ptp_controller_utils as PCU
    from hedit.p2p.ptp_classes import ControllerBatch
    from hedit.p2p.ptp_utils import register_attention_control
    cs = []
    for pi in pis:
        s_, t_, bw, is_replace = PROMPT_PAIRS[pi]
        cs.append(PCU.make_controller(prompts=[s_, t_], is_replace_controller=is_replace, cross_replace_steps=0.4, self_replace_steps=0.35,
                                      blend_word=((bw[0],), (bw[1],)) if bw else None,
                                      equilizer_params={"words": (bw[1],), "values": (2.0,)} if bw else None, num_steps=num_steps,
                                      tokenizer=hip.tokenizer, device=hip.device))
    c = cs[0] if len(cs) == 1 else ControllerBatch(cs)
    register_attention_control(hip, c)
    return c


@pytest.mark.parametrize("mode", ["ef_p2p", "pnp_inv_p2p", "ef_masactrl", "pnp_inv_masactrl"])
def test_run_direct_is_batch_invariant(full_gain, mode):
    """three images in lock-step give, row by row, the bits of three one-image runs"""
    from hedit.engine import HEditEngine
    from hedit.masactrl import MutualSelfAttentionControl, regiter_attention_editor_diffusers
    from hedit.scheduler import DDIMScheduler
    hip = full_gain
    ddim, masa = mode.startswith("pnp_inv"), mode.endswith("masactrl")
    Tn, n, pis = 6, 3, (0, 2, 1)
    saved = hip.scheduler
    try:
        hip.scheduler = DDIMScheduler(steps_offset=0) if ddim else DDIMScheduler()
        hip.scheduler.set_timesteps(Tn)
        eng = HEditEngine(hip)
        pairs = [["" if masa else PROMPT_PAIRS[pi][0], PROMPT_PAIRS[pi][1]] for pi in pis]
        w0 = _images(n, 300)
        if ddim:
            _, zs, xts = eng.ddim_inversion(w0, [p[0] for p in pairs], 1.0)
        else:
            zs, xts = eng.ddpm_inversion(w0, [p[0] for p in pairs], eta=1.0, cfg_src=1.0, generator=torch.Generator(device=G.dev()).manual_seed(3))

        def run(rows):
            if masa:
                c = MutualSelfAttentionControl(1, 0)
                regiter_attention_editor_diffusers(hip, c)
            else:
                c = _batch_controller(hip, [pis[i] for i in rows], Tn)
            out = eng.run_direct(xts[Tn][rows].contiguous(), zs[:, rows].contiguous(), [pairs[i] for i in rows], CFG, c, eta=1.0,
                                 after_skip_steps=Tn, ddim_inv=ddim)
            assert c.cur_step == Tn
            return out
        e_all, r_all = run([0, 1, 2])
        for i in range(n):
            e1, r1 = run([i])
            G.sync()
            assert torch.equal(e_all[i:i + 1], e1) and torch.equal(r_all[i:i + 1], r1), i
        assert torch.isfinite(e_all).all() and G.rel_err(e_all, r_all) > 1e-2
    finally:
        hip.scheduler = saved
        hip.unet._attention_editor = None


def test_run_direct_pnp_is_batch_invariant():
    from hedit.engine import HEditEngine
    from hedit.plug_n_play import register_attention_control_efficient, register_conv_control_efficient
    from hedit.scheduler import DDIMScheduler
    Tp, n = 4, 3
    hip, _, _ = make_pair(TINY4_CONFIG, Tp, out_scale=0.3)
    hip.scheduler = DDIMScheduler(steps_offset=0)
    hip.scheduler.set_timesteps(Tp)
    register_attention_control_efficient(hip, hip.scheduler.timesteps[:3])
    register_conv_control_efficient(hip, hip.scheduler.timesteps[:2])
    eng = HEditEngine(hip)
    pairs = [list(PROMPT_PAIRS[pi][:2]) for pi in (0, 1, 2)]
    xT = _images(n, 500, 64)
    kw = dict(eta=0.0, after_skip_steps=Tp, ddim_inv=False, uncond="src")
    e_all, r_all = eng.run_direct_pnp(xT, None, pairs, [7.5, 7.5], **kw)
    for i in range(n):
        e1, r1 = eng.run_direct_pnp(xT[i:i + 1], None, [pairs[i]], [7.5, 7.5], **kw)
        G.sync()
        assert torch.equal(e_all[i:i + 1], e1) and torch.equal(r_all[i:i + 1], r1), i
    assert torch.isfinite(e_all).all() and G.rel_err(e_all, r_all) > 1e-2


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("masa", [False, True])
def test_edit_friendly_reconstruction_is_exact(full_gain, n, masa):
    """What makes EF edit friendly: the source row of run_direct, fed the inversion's noise maps, retraces the inverted
    trajectory BIT FOR BIT (full-gain network, 10 steps) -- the source rows of the controlled pass carry the bits of a plain
    pass and hedit_step_pair shares ddpm_mu with hedit_step_invert.  With MasaCtrl the source prompt is "", so e_c and e_u of
    the source row are the same bits too."""
    from hedit.engine import HEditEngine
    from hedit.masactrl import MutualSelfAttentionControl, regiter_attention_editor_diffusers
    hip = full_gain
    Tn = 10
    hip.scheduler.set_timesteps(Tn)
    eng = HEditEngine(hip)
    pis = [i % len(PROMPT_PAIRS) for i in range(n)]
    pairs = [["" if masa else PROMPT_PAIRS[pi][0], PROMPT_PAIRS[pi][1]] for pi in pis]
    w0 = _images(n, 40 + n)
    zs, xts = eng.ddpm_inversion(w0, [p[0] for p in pairs], eta=1.0, cfg_src=1.0, generator=torch.Generator(device=G.dev()).manual_seed(40 + n))
    try:
        if masa:
            c = MutualSelfAttentionControl(2, 0)
            regiter_attention_editor_diffusers(hip, c)
        else:
            c = _batch_controller(hip, pis, Tn)
        edit, recon = eng.run_direct(xts[Tn].contiguous(), zs, pairs, CFG, c, eta=1.0, after_skip_steps=Tn, ddim_inv=False)
        G.sync()
    finally:
        hip.unet._attention_editor = None
    assert torch.isfinite(edit).all()
    print("ef exact recon", "masactrl" if masa else "p2p", n, "max |recon - xts[0]|", G.max_err(recon, xts[0]))
    assert torch.equal(recon, xts[0])
    assert G.rel_err(recon, w0) < 2e-6
    assert G.rel_err(edit, recon) > 1e-2


# ------------------------------------------------------------------------------------------ 6: the driver
def _driver():
    sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
    spec = importlib.util.spec_from_file_location("hedit_main_baselines", os.path.join(ROOT, "h-edit_amd", "main_baselines.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


MODE_FLAGS = {"ef": ["--eta", "1.0", "--skip", "1"], "ef_p2p": ["--eta", "1.0"], "pnp_inv_p2p": ["--eta", "0.0", "--sa", "0.6"],
              "ef_masactrl": ["--eta", "1.0", "--step", "1", "--layer", "2"], "pnp_inv_masactrl": ["--eta", "0.0", "--step", "1", "--layer", "2"],
              "np_pnp": ["--eta", "0.0", "--pnp_f_t", "0.5", "--pnp_attn_t", "0.75"]}
NAME_TAIL = {"ef": "_", "ef_p2p": "_xa_0.4_sa0.35_", "pnp_inv_p2p": "_xa_0.4_sa0.6_", "ef_masactrl": "_step_1_layer_2_",
             "pnp_inv_masactrl": "_step_1_layer_2_", "np_pnp": "_f_t_0.5_attn_t_0.75_"}


@pytest.mark.parametrize("mode", list(MODE_FLAGS))
def test_driver_writes_edited_images(tmp_path, mode):
    """every mode from a PIE-Bench-style mapping file to 256 x 256 PNGs; the modes on a DDIM inversion (no random numbers
    drawn) also with --batch 2: byte-identical images"""
    from PIL import Image
    d = _dataset(tmp_path)
    common = ["--data_path", str(d), "--random_init", "--tiny", "--num_diffusion_steps", "4", "--edit_category_list", "0", "1",
              "--mode", mode] + MODE_FLAGS[mode]
    one = _driver().main(common + ["--output_path", str(tmp_path / "r1")])
    assert len(one) == 2                           # category 7 filtered out
    for p in one:
        sub = os.path.relpath(p, str(tmp_path / "r1")).split(os.sep)[0]
        assert sub.startswith(f"{mode}_total_steps_4_skip_{1 if mode == 'ef' else 0}_implicit_False_eta_") and sub.endswith(NAME_TAIL[mode]), sub
        im = np.array(Image.open(p))
        assert im.shape == (256, 256, 3) and im.std() > 0
    if "--eta" in common and common[common.index("--eta") + 1] == "0.0":
        two = _driver().main(common + ["--output_path", str(tmp_path / "r2"), "--batch", "2"])
        assert len(two) == 2
        for a, b in zip(sorted(one), sorted(two)):
            assert os.path.basename(a) == os.path.basename(b)
            assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b)))


@pytest.mark.parametrize("mode,eta", [("nmg_p2p", "0.0"), ("ef_pnp", "1.0"), ("nt_pnp", "0.0"), ("h_edit_R_p2p", "1.0")])
def test_driver_refuses_what_is_not_built(tmp_path, mode, eta):
    with pytest.raises(NotImplementedError) as ei:
        _driver().main(["--data_path", str(tmp_path), "--random_init", "--tiny", "--mode", mode, "--eta", eta])
    assert mode in str(ei.value) and len(str(ei.value)) > 40         # says why
    with pytest.raises(AssertionError):
        _driver().main(["--data_path", str(tmp_path), "--random_init", "--tiny", "--mode", "pnp_inv_p2p", "--eta", "1.0"])
