"""Edit Friendly / PnP Inversion with MasaCtrl -- drop-in for text-guided/inversion/masactrl_baselines.py:15-94
(``ef_or_pnp_inv_w_masactrl``): the direct-sampling loop of p2p_baselines under the mutual-self-attention editor
registered on the model (``regiter_attention_editor_diffusers``); no LocalBlend.  Same signature, defaults,
assertion and return values."""
from ..engine import HEditEngine
from .p2p_baselines import _etas, _latents


def ef_or_pnp_inv_w_masactrl(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None,
                             is_ddim_inversion=False):
    assert len(prompts) >= 2, "require both source and target prompts"
    editor = getattr(model.unet, "_attention_editor", None)
    if editor is None:
        raise RuntimeError("register an editor first: regiter_attention_editor_diffusers(model, MutualSelfAttentionControl(...))")
    eta = _etas(model, etas)
    x, z = _latents(xT, zs)
    return HEditEngine(model).run_direct(x, z, [list(prompts[:2])], [float(cfg_scales[0]), float(cfg_scales[1])], editor,
                                         eta=eta, after_skip_steps=zs.shape[0], ddim_inv=is_ddim_inversion)
