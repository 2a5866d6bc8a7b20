"""Comparison editors with Plug-and-Play injection -- drop-in for text-guided/inversion/pnp_baselines.py:
nmg_pnp :32-126, nulltext_pnp :134-236, negative_prompt_pnp :244-309 and ef_or_pnp_inv_w_pnp :317-393 (``register_time``
:10-24 lives in hedit.plug_n_play.pnp_utils).  Same signatures, defaults, assertions and return values; the injection
schedules are the ones registered on the model.  nmg_pnp differentiates a plain UNet pass with respect to its input (host
code, see p2p_baselines.nmg_p2p); nulltext_pnp differentiates it with respect to the text context -- on the HIP pipeline
a ``UNet2DConditionModel(grad="context")``, whose backward is the executor's hedit_unet_backward_ctx."""
import torch
import torch.nn.functional as F

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


def nulltext_pnp(model, xT, xT_ori, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, optimization_steps=10,
                 epsilon=1e-5, per_image=False, register_time=None):
    """Null-text inversion with Plug-and-Play.  Per step i: register_time; the source-conditional eps of the reconstruction
    row, silent and without grad (:194-195); a FRESH Adam (lr = 1e-2 (1 - i / 100)) on the detached null embedding (:199-200
    -- the reference detaches without copying, so Adam's in-place updates land in the encoder's output and step i + 1 starts
    from step i's optimised embedding with a new optimiser state; the same here, on a copy made once); up to optimization_steps
    updates of mse(reverse_step(eps_u + cfg_tar (eps_c - eps_u)), xT_ori[len - i - 2]) with the reference's stop
    ``loss < epsilon + i * 2e-5`` checked after the update (:202-215); then the two unconditional rows with the optimised
    embedding, silent, and the [source, target] pair under the registered injection, both rows guided with cfg_tar
    (:219-228), eta = 0 steps.  per_image (addition): n [source, target] pairs in lock-step -- one embedding, one optimiser
    state and one loss per image; an image that met the stop is frozen and the gradient pass runs on the still-active rows
    only, so on a batch-invariant model image j is its single run.  ``register_time``: as in nmg_pnp.  The loss is taken
    through this module's name ``F``, as in the reference module.  Returns (edited latent, reconstructed latent)."""
    from .inversion_utils import reverse_step
    assert len(prompts) >= 2 and etas == 0, "PnP requires source and target prompts, with eta is set to 0 for NT"
    tell_time = register_time if register_time is not None else globals()["register_time"]
    n, xt, text, uncond, cfg_tar, op = _nmg_setup(model, xT, etas, prompts, cfg_scales, zs)
    if n > 1 and not per_image:
        raise ValueError("n images in lock-step need per_image=True: one embedding and one optimiser per image")
    embs = [uncond[j:j + 1].detach().clone().requires_grad_(True) for j in range(n)]
    for i, t in enumerate(op):
        x_rec = xt[:n]
        x_ori = xT_ori[len(xT_ori) - i - 2].to(xt.device).reshape(x_rec.shape)
        tell_time(model, t.item() if torch.is_tensor(t) else int(t))
        with torch.no_grad():
            e_c = _silent_pass(model, x_rec, t, text[:n])
        with torch.enable_grad():
            opts = [torch.optim.Adam([e], lr=1e-2 * (1. - i / 100.)) for e in embs]
            active = list(range(n))
            for _ in range(optimization_steps):
                if not active:
                    break
                rows = torch.tensor(active, device=xt.device)
                whole = len(active) == n
                xa = x_rec if whole else x_rec[rows]
                e_u = _silent_pass(model, xa, t, torch.cat([embs[j] for j in active]))
                e = e_u + cfg_tar * ((e_c if whole else e_c[rows]) - e_u)
                pred = reverse_step(model, e, t, xa, eta=0.0, variance_noise=None)
                # one mean per image, each over its own elements: the reference's loss for one image, and in a lock-step
                # batch the same number as in the image's single run
                per = [F.mse_loss(pred[k:k + 1], x_ori[j:j + 1]) for k, j in enumerate(active)]
                for j in active:
                    opts[j].zero_grad()
                torch.stack(per).sum().backward()
                still = []
                for k, j in enumerate(active):
                    opts[j].step()
                    if not per[k].item() < epsilon + i * 2e-5:
                        still.append(j)
                active = still
        with torch.no_grad():
            emb = torch.cat([e.detach() for e in embs])
            e_u = torch.cat([_silent_pass(model, xt[:n], t, emb), _silent_pass(model, xt[n:], t, emb)])
            e_c = _pair_pass(model, xt, t, text, n)
            e = e_u + cfg_tar * (e_c - e_u)
            xt = reverse_step(model, e, t, xt, eta=0.0, variance_noise=None)
    return xt[n:], xt[:n]
