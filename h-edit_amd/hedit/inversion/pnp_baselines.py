"""Comparison editors with Plug-and-Play injection -- drop-in for text-guided/inversion/pnp_baselines.py:
nmg_pnp :32-126, negative_prompt_pnp :244-309 and ef_or_pnp_inv_w_pnp :317-393 (``register_time`` :10-24 lives in
hedit.plug_n_play.pnp_utils).  Same signatures, defaults, assertions and return values; the injection schedules are
the ones registered on the model.  nmg_pnp differentiates a plain UNet pass with respect to its input (host code, see
p2p_baselines.nmg_p2p).  nulltext_pnp (:134-236) needs the gradient with respect to the text context and is not
provided."""
import torch

from ..engine import HEditEngine
from ..plug_n_play.pnp_utils import register_time  # noqa: F401  (the reference module defines it too)
from .p2p_baselines import _etas, _latents, _nmg_guide, _nmg_setup, _silent_pass


def negative_prompt_pnp(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None):
    """Negative-prompt inversion: the unconditional rows are evaluated with the SOURCE embedding (:293-294) and both
    rows are guided with cfg_tar (:301-302); deterministic steps; zs only sets the number of steps."""
    assert len(prompts) >= 2 and etas == 0, "PnP requires source and target prompts, with eta is set to 0"
    eta = _etas(model, etas)
    x, _ = _latents(xT, zs)
    w = float(cfg_scales[1])
    return HEditEngine(model).run_direct_pnp(x, None, list(prompts[:2]), [w, w], eta=eta, after_skip_steps=zs.shape[0],
                                             ddim_inv=False, uncond="src")


def ef_or_pnp_inv_w_pnp(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, is_ddim_inversion=False):
    """The same loop with the null embedding on the unconditional rows and (cfg_src, cfg_tar).  The reference asserts
    etas == 0 here (:338) although its docstring and its driver (main_plugnplay.py) ask for 1.0, so its `ef_pnp` /
    `pnp_inv_w_pnp` modes stop at this assertion; the assertion is kept as it is."""
    assert len(prompts) >= 2 and etas == 0, "PnP requires source and target prompts, with eta is set to 0"
    eta = _etas(model, etas)
    x, z = _latents(xT, zs)
    return HEditEngine(model).run_direct_pnp(x, z, list(prompts[:2]), [float(cfg_scales[0]), float(cfg_scales[1])], eta=eta,
                                             after_skip_steps=zs.shape[0], ddim_inv=is_ddim_inversion, uncond="null")


def _pair_pass(model, xt, t, text, n):
    """the [source]*n, [target]*n pass under the registered injection; n > 1 on the HIP pipeline: the editor's lock-step
    plan (row n + i takes from row i), as HEditEngine.run_direct_pnp asks for it"""
    unet = model.unet
    editor = getattr(unet, "_attention_editor", None)
    if n == 1 or editor is None or not hasattr(unet, "forward_raw"):
        return unet(xt, t, encoder_hidden_states=text).sample
    e = unet.forward_raw(xt.contiguous(), float(t), text.contiguous(), editor._plan(unet, 2 * n, xt.shape[2], xt.shape[3], True, n_images=n))
    editor._after_pass(True)
    return e


def nmg_pnp(model, xT, xT_ori, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, guidance_noise_map=10.0,
            grad_scale=5e+3, per_image=False, register_time=None):
    """Noise Map Guidance with Plug-and-Play.  Per step: register_time, the guidance update of the reconstruction row
    (p2p_baselines._nmg_guide) from an unconditional pass the injection hooks stay silent to, then THREE passes --
    the two unconditional rows on their own, again silent, and the [source, target] pair under the registered
    injection (:109-113) --, both rows guided with cfg_tar (:117-118), eta = 0 steps.  ``register_time`` (addition):
    the function that tells the model's hooks the timestep, by default this module's (a torch model with the
    reference's hooks passes the reference's).  Returns (edited latent, reconstructed latent)."""
    from .inversion_utils import reverse_step
    assert len(prompts) >= 2 and etas == 0, "PnP requires source and target prompts, with eta is set to 0 for NMG"
    tell_time = register_time if register_time is not None else globals()["register_time"]
    n, xt, text, uncond, cfg_tar, op = _nmg_setup(model, xT, etas, prompts, cfg_scales, zs)
    for i, t in enumerate(op):
        x_rec, x_tar = xt.chunk(2)
        tell_time(model, t.item() if torch.is_tensor(t) else int(t))
        x_rec = _nmg_guide(model, x_rec, xT_ori[len(xT_ori) - i - 2], t, lambda x: _silent_pass(model, x, t, uncond[:n]),
                           guidance_noise_map, grad_scale, per_image)
        xt = torch.cat([x_rec, x_tar])
        with torch.no_grad():
            e_u = torch.cat([_silent_pass(model, xt[:n], t, uncond[:n]), _silent_pass(model, xt[n:], t, uncond[n:])])
            e_c = _pair_pass(model, xt, t, text, n)
            e = e_u + cfg_tar * (e_c - e_u)
            xt = reverse_step(model, e, t, xt, eta=0.0, variance_noise=None)
    return xt[n:], xt[:n]
