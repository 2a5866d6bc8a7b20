"""fp32 twins of the gradient-free comparison editors, written on the oracle's primitives (oracle.loops.encode_text,
oracle.sched.reverse_step, the processors registered by oracle.p2p.register / oracle.masactrl.register_editor /
oracle.pnp.register_pnp).  They restate
  ef_wo_p2p, ef_or_pnp_inv_w_p2p     text-guided/inversion/p2p_baselines.py:19-95, 103-187
  ef_or_pnp_inv_w_masactrl           text-guided/inversion/masactrl_baselines.py:15-94
  negative_prompt_pnp, ef_or_pnp_inv_w_pnp   text-guided/inversion/pnp_baselines.py:244-309, 317-393
and are PINNED on vectors from running those modules (tests/test_oracle_baselines.py, g18).  They live under tests/
because oracle/ is frozen.  The three paired loops share one skeleton; what differs is how the four eps rows of a step
are evaluated."""
import torch

from oracle import pnp as OPNP
from oracle import sched as S
from oracle.loops import encode_text


def _etas(sch, etas):
    if etas is None:
        etas = 0
    if type(etas) in (int, float):
        etas = [etas] * sch.num_inference_steps
    assert len(etas) == sch.num_inference_steps
    return etas


def _unet(model, x, t, ctx, kw=None):
    with torch.no_grad():
        if kw is None:
            return model.unet(x, t, encoder_hidden_states=ctx).sample
        return model.unet(x, t, encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample


def _start(model, xT, zs, rows):
    sch = model.scheduler
    T, A = sch.num_inference_steps, zs.shape[0]
    x = xT.unsqueeze(0) if xT.dim() < 4 else xT
    xt = torch.cat([x] * rows)
    op = [int(t) for t in sch.timesteps[-A:]]
    idx = [T - i - (T - A + 1) for i in range(A)]
    return sch, xt, op, idx


def ef_wo_p2p(model, xT, etas=0, prompts="", cfg_scales=None, zs=None, controller=None, is_ddim_inversion=False):
    """one latent, prompts = [target]: two plain 1-row passes per step, the controller's callback once at the end"""
    sch, xt, op, idx = _start(model, xT, zs, 1)
    etas = _etas(sch, etas)
    txt, unc = encode_text(model, prompts), encode_text(model, [""])
    w = float(cfg_scales[0])
    off = {"use_controller": False}
    for i, t in enumerate(op):
        e_u = _unet(model, xt, t, unc, off)
        e_c = _unet(model, xt, t, txt, off)
        xt = S.reverse_step(sch, e_u + w * (e_c - e_u), t, xt, eta=etas[idx[i]], z=zs[idx[i]], ddim_inv=is_ddim_inversion)
    if controller is not None:
        xt = controller.step_callback(xt)
    return xt


def _paired(model, xT, etas, prompts, w_src, w_tar, zs, ddim_inv, eps_rows, callback=None, use_z=True):
    """eps_rows(xt, t) -> (e_u_src, e_u_tar, e_c_src, e_c_tar).  Source row: (w_src, eta, z); target row: (w_tar, eta
    or 0 for a DDIM inversion, the same z)."""
    assert len(prompts) >= 2
    sch, xt, op, idx = _start(model, xT, zs, 2)
    etas = _etas(sch, etas)
    for i, t in enumerate(op):
        e_us, e_ut, e_cs, e_ct = eps_rows(xt, t)
        z = zs[idx[i]] if use_z else None
        eta = etas[idx[i]]
        x0 = S.reverse_step(sch, e_us + w_src * (e_cs - e_us), t, xt[0], eta=eta, z=z, ddim_inv=ddim_inv)
        x1 = S.reverse_step(sch, e_ut + w_tar * (e_ct - e_ut), t, xt[1], eta=0 if ddim_inv else eta, z=z, ddim_inv=ddim_inv)
        xt = torch.cat([x0, x1])
        if callback is not None:
            xt = callback(xt)
    return xt[1].unsqueeze(0), xt[0].unsqueeze(0)


def _controlled_rows(model, prompts):
    """the 4-row pass [x_s|null, x_t|null, x_s|src, x_t|tar] under whatever processors are registered (no kwargs:
    control on, save_attn at its default True)"""
    ctx = torch.cat([encode_text(model, [""] * 2), encode_text(model, list(prompts[:2]))])

    def rows(xt, t):
        e = _unet(model, torch.cat([xt] * 2), t, ctx)
        return e[0:1], e[1:2], e[2:3], e[3:4]
    return rows


def ef_or_pnp_inv_w_p2p(model, xT, etas=0, prompts="", cfg_scales=None, zs=None, controller=None, is_ddim_inversion=False):
    cb = controller.step_callback if controller is not None else None
    return _paired(model, xT, etas, prompts, float(cfg_scales[0]), float(cfg_scales[1]), zs, is_ddim_inversion,
                   _controlled_rows(model, prompts), cb)


def ef_or_pnp_inv_w_masactrl(model, xT, etas=0, prompts="", cfg_scales=None, zs=None, is_ddim_inversion=False):
    return _paired(model, xT, etas, prompts, float(cfg_scales[0]), float(cfg_scales[1]), zs, is_ddim_inversion,
                   _controlled_rows(model, prompts))


def _pnp_rows(model, prompts, uncond_is_source):
    txt = encode_text(model, list(prompts[:2]))
    unc = txt[0:1] if uncond_is_source else encode_text(model, [""])

    def rows(xt, t):
        OPNP.register_time(model, t)
        e_us = _unet(model, xt[0:1], t, unc)          # one row: the hooks stay silent
        e_ut = _unet(model, xt[1:2], t, unc)
        e = _unet(model, xt, t, txt)                  # two rows: injection
        return e_us, e_ut, e[0:1], e[1:2]
    return rows


def negative_prompt_pnp(model, xT, etas=0, prompts="", cfg_scales=None, zs=None):
    assert etas == 0
    w = float(cfg_scales[1])                          # cfg_tar on BOTH rows
    return _paired(model, xT, 0, prompts, w, w, zs, False, _pnp_rows(model, prompts, True), use_z=False)


def ef_or_pnp_inv_w_pnp(model, xT, etas=0, prompts="", cfg_scales=None, zs=None, is_ddim_inversion=False):
    assert etas == 0
    return _paired(model, xT, etas, prompts, float(cfg_scales[0]), float(cfg_scales[1]), zs, is_ddim_inversion,
                   _pnp_rows(model, prompts, False))
