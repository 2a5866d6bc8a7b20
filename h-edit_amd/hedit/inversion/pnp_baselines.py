"""Gradient-free comparison editors with Plug-and-Play injection -- drop-in for text-guided/inversion/pnp_baselines.py:
negative_prompt_pnp :244-309 and ef_or_pnp_inv_w_pnp :317-393 (``register_time`` :10-24 lives in
hedit.plug_n_play.pnp_utils).  Same signatures, defaults, assertions and return values; the injection schedules are
the ones registered on the model.  nmg_pnp (:32-126) and nulltext_pnp (:134-236) differentiate through the UNet and
are not provided."""
from ..engine import HEditEngine
from ..plug_n_play.pnp_utils import register_time  # noqa: F401  (the reference module defines it too)
from .p2p_baselines import _etas, _latents


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
