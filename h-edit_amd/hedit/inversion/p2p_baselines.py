"""Gradient-free comparison editors on the P2P path -- drop-in for text-guided/inversion/p2p_baselines.py:
ef_wo_p2p :19-95 (Edit Friendly alone) and ef_or_pnp_inv_w_p2p :103-187 (Edit Friendly / PnP Inversion with P2P).
Same signatures, defaults, assertions and return values; one controlled UNet pass per step and the paired step
kernel (hedit.engine.HEditEngine.run_direct with one image).  As in the other wrappers of this package the
``controller`` argument is both the attention control of the pass and the LocalBlend callback.  nmg_p2p (:195-293)
needs the gradient of a UNet pass with respect to its input and is not provided."""
from ..engine import HEditEngine


def _etas(model, etas):
    if etas is None:
        etas = 0
    if type(etas) in [int, float]:
        etas = [etas] * model.scheduler.num_inference_steps
    assert len(etas) == model.scheduler.num_inference_steps
    etas = [float(e) for e in etas]
    return etas[0] if all(e == etas[0] for e in etas) else etas


def _latents(xT, zs):
    x = xT.unsqueeze(0) if xT.dim() < 4 else xT
    return x, zs[:, None]            # (1,C,H,W), (T',1,C,H,W)


def ef_wo_p2p(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, controller=None,
              is_ddim_inversion=False):
    """prompts = [target]; cfg_scales = [cfg_tar].  Returns ONE tensor, the edited latent, as the reference does
    (p2p_baselines.py:95) -- its own driver unpacks two values from it (main_p2p.py:250) and raises ValueError; the
    quirk is kept so that callers written against the reference function see the same value.  The controller is not
    applied to the passes (`use_controller: False`, :66); its step_callback runs once, after the loop (:92-93)."""
    if isinstance(prompts, str) or len(prompts) != 1:
        raise NotImplementedError("ef_wo_p2p edits one image with one target prompt: prompts = [target]")
    eta = _etas(model, etas)
    x, z = _latents(xT, zs)
    edit, _ = HEditEngine(model).run_direct(x, z, [[prompts[0]]], [float(cfg_scales[0])], controller, eta=eta,
                                            after_skip_steps=zs.shape[0], ddim_inv=is_ddim_inversion, control=False)
    return edit


def ef_or_pnp_inv_w_p2p(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, controller=None,
                        is_ddim_inversion=False):
    """prompts = [source, target]; cfg_scales = [cfg_src, cfg_tar]; is_ddim_inversion: False = Edit Friendly (both rows
    stochastic with etas), True = PnP Inversion (source row replays the stored corrections, target row eta = 0).
    Returns (edited latent, reconstructed latent)."""
    assert len(prompts) >= 2, "for prompt-to-prompt, requires both source and target prompts"
    eta = _etas(model, etas)
    x, z = _latents(xT, zs)
    return HEditEngine(model).run_direct(x, z, [list(prompts[:2])], [float(cfg_scales[0]), float(cfg_scales[1])], controller,
                                         eta=eta, after_skip_steps=zs.shape[0], ddim_inv=is_ddim_inversion)
