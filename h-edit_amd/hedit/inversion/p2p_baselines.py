"""Comparison editors on the P2P path -- drop-in for text-guided/inversion/p2p_baselines.py:
ef_wo_p2p :19-95 (Edit Friendly alone), ef_or_pnp_inv_w_p2p :103-187 (Edit Friendly / PnP Inversion with P2P) and
nmg_p2p :195-293 (Noise Map Guidance with P2P).  Same signatures, defaults, assertions and return values.  The two
gradient-free ones are one controlled UNet pass per step and the paired step kernel
(hedit.engine.HEditEngine.run_direct with one image); as in the other wrappers of this package their ``controller``
argument is both the attention control of the pass and the LocalBlend callback.  nmg_p2p differentiates a plain UNet
pass with respect to its input: host code over ``model.unet`` that runs on any differentiable model -- on the HIP
pipeline a ``UNet2DConditionModel(grad=True)``, whose backward is the executor's input-gradient pass."""
import torch

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


# ---------------------------------------------------------------------------------------------- Noise Map Guidance
def _nmg_setup(model, xT, etas, prompts, cfg_scales, zs):
    """the prologue the two NMG loops share.  prompts: [source, target], or one such pair per image for n images in
    lock-step (xT (n,C,H,W), xT_ori (T'+1,n,C,H,W)).  Rows are kind-major like the engine's: [source]*n, [target]*n."""
    from .inversion_utils import encode_text
    pairs = [list(prompts[:2])] if isinstance(prompts[0], str) else [list(p[:2]) for p in prompts]
    n = len(pairs)
    if xT.dim() < 4:
        xT = xT.unsqueeze(0)
    if xT.shape[0] != n:
        raise ValueError("one [source, target] pair per image expected")
    _etas(model, etas)                                    # one eta per inference step, as the reference checks
    # every image's prompts as the reference's batch of two, so that an embedding has the bits of the single run whatever it is
    # batched with (a torch text encoder's matrix products pick batch-dependent kernels)
    per = [encode_text(model, p) for p in pairs]
    text = torch.cat([e[:1] for e in per] + [e[1:] for e in per])
    null = encode_text(model, [""] * 2)
    uncond = torch.cat([null[:1]] * n + [null[1:]] * n)
    cfg_tar = torch.tensor([float(c) for c in cfg_scales]).view(-1, 1, 1, 1).to(xT.device).chunk(2)[1]
    op = list(model.scheduler.timesteps[-zs.shape[0]:])
    return n, torch.cat([xT, xT]), text, uncond, cfg_tar, op


def _silent_pass(model, x, t, emb):
    """A pass that no controller or injection hook touches.  The HIP facade is told so; a torch model with the
    reference's hooks gets one row at a time, to which they stay silent (pnp_baselines.py:93)."""
    if hasattr(model.unet, "forward_raw"):
        return model.unet(x, t, encoder_hidden_states=emb, cross_attention_kwargs={"use_controller": False, "use_editor": False}).sample
    return torch.cat([model.unet(x[j:j + 1], t, encoder_hidden_states=emb[j:j + 1]).sample for j in range(x.shape[0])])


def _nmg_guide(model, x_rec, x_ori, t, eps_of, guidance_noise_map, grad_scale, per_image):
    """One noise-map-guidance update of the reconstruction rows (p2p_baselines.py:249-266): the unconditional eps at
    x_rec, the gradient of |reverse_step(eps, x_rec) - x_ori|_1 with respect to x_rec, eps pushed along it, one eta = 0
    step.  per_image: the L1 mean is taken per image (the reference's is over the batch, which is one image there), so
    entry j of a lock-step batch is updated exactly as it would be alone."""
    from ..engine import Schedule
    from .inversion_utils import reverse_step
    with torch.enable_grad():
        x_in = x_rec.detach().requires_grad_(True)
        eps = eps_of(x_in)
        pred = reverse_step(model, eps, t, x_in, eta=0.0, variance_noise=None)
        x_ori = x_ori.to(pred.device)
        if per_image:
            loss = (pred - x_ori.reshape(pred.shape)).abs().flatten(1).mean(1).sum()
        else:
            loss = torch.nn.functional.l1_loss(pred, x_ori)
        grad = -torch.autograd.grad(loss, x_in)[0]
    eps = eps.detach()
    a_t = Schedule(model.scheduler).ab[int(t)]
    eps_cond = eps - float((1 - a_t) ** 0.5) * grad * grad_scale
    eps = eps + guidance_noise_map * (eps_cond - eps)
    return reverse_step(model, eps, t, x_rec, eta=0.0, variance_noise=None)


def nmg_p2p(model, xT, xT_ori, etas=0.0, prompts="", cfg_scales=None, prog_bar=False, zs=None, controller=None,
            guidance_noise_map=10.0, grad_scale=5e+3, per_image=False):
    """Noise Map Guidance with P2P.  xT_ori: the latents of the DDIM inversion, x_0 first (xT_ori[len - i - 2] is the
    ground truth of step i, :250); zs only sets the number of steps.  Per step: the guidance update of the
    reconstruction row from a plain unconditional pass, then one controlled four-row pass whose BOTH rows are guided with
    cfg_tar (:280-281), eta = 0 steps, the controller's step_callback.  per_image (addition): n images in lock-step,
    see _nmg_guide.  Returns (edited latent, reconstructed latent)."""
    from .inversion_utils import reverse_step
    assert len(prompts) >= 2 and etas == 0, "P2P requires source and target prompts, with eta is set to 0 for NMG"
    n, xt, text, uncond, cfg_tar, op = _nmg_setup(model, xT, etas, prompts, cfg_scales, zs)
    plain = {"use_controller": False}
    for i, t in enumerate(op):
        x_rec, x_tar = xt.chunk(2)
        x_rec = _nmg_guide(model, x_rec, xT_ori[len(xT_ori) - i - 2], t,
                           lambda x: model.unet(x, t, encoder_hidden_states=uncond[:n], cross_attention_kwargs=plain).sample,
                           guidance_noise_map, grad_scale, per_image)
        xt = torch.cat([x_rec, x_tar])
        with torch.no_grad():
            e = model.unet(torch.cat([xt] * 2), t, encoder_hidden_states=torch.cat([uncond, text])).sample
            e_u, e_c = e.chunk(2)
            e = e_u + cfg_tar * (e_c - e_u)
            xt = reverse_step(model, e, t, xt, eta=0.0, variance_noise=None)
            if controller is not None:
                xt = controller.step_callback(xt)
    return xt[n:], xt[:n]
