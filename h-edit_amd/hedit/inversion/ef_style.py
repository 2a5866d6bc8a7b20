"""Edit Friendly with P2P for the combined text + style task -- drop-in for text-guided-n-style/inversion/ef.py:14-132
(``ef_p2p``), the comparison column of that task (main_edit.py:218-223).  Same signature, defaults, assertions and return
values (edited latent, reconstructed latent).  Per step: one controlled four-row pass [u_src, u_tar, c_src, c_tar] with
cfg_scales = [cfg_src, cfg_tar] and the reverse step of both rows on the shared noise z (under ``is_ddim_inversion`` the
target row steps with eta = 0, :86-87, kept as written); then the style step on the target latent, which differentiates
||Gram residual|| of the decoded Tweedie estimate THROUGH a plain two-row pass [x|uncond, x|tar] of the eps-network (the
controller's step counter does not advance), rho = rms(e_c - e_u) of that plain pass / rms(g) * weight_edit_clip; the
controller's step_callback.

The loop is host code over ``model.unet`` / ``model.vae`` that runs on any differentiable model (the tiny torch models of the
tests on the CPU).  On the HIP pipeline -- a ``UNet2DConditionModel(grad=True)`` -- the style step is
``HEditEngine.ef_style_step``: the executor's input-gradient pass with the latent-side arithmetic in two kernels and no host
wait, where the reference reads two ``.item()``.

Additions: ``per_image=True`` runs n images in lock-step -- ``prompts`` = one [source, target] pair per image, ``image_encoder``
= one encoder per image, xT (n,C,H,W), zs (T',n,C,H,W); every image is edited exactly as it would be alone (the rho means are
per image, which for one image is the reference's mean).  ``fused``: None = the fused step on a HIP model and torch autograd
elsewhere; False = the torch-autograd restatement everywhere (on a HIP model through ``_EpsGrad``, the decoder's node and the
encoder)."""
import torch

from .inversion_utils import encode_text, reverse_step, reverse_step_pred_x0


def _is_hip(model):
    return hasattr(model.unet, "forward_raw")


def ef_style_update(model, image_encoder, x, x_prev, uncond, text, t, w_tar, weight, fused=None, engine=None):
    """x_prev - rho g for the n target latents x at timestep t (ef.py:91-124).  uncond / text (n,77,D): the null and the
    target embeddings; image_encoder: one object, or one per image (its get_gram_matrix_residual reads batch item 0)."""
    hip = _is_hip(model)
    if fused is None:
        fused = hip
    if fused:
        if not hip:
            raise RuntimeError("fused=True: the fused style step runs on the HIP UNet only")
        if engine is None:
            from ..engine import HEditEngine
            engine = HEditEngine(model)
        return engine.ef_style_step(x.contiguous(), x_prev.contiguous(), uncond.contiguous(), text.contiguous(), int(t),
                                    float(w_tar), image_encoder, weight)
    n = x.shape[0]
    encs = list(image_encoder) if isinstance(image_encoder, (list, tuple)) else [image_encoder] * n
    # a pass no controller touches; the torch models' processors take the reference's one switch
    plain = {"use_controller": False, "use_editor": False} if hip else {"use_controller": False}
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        e = model.unet(torch.cat([xg] * 2), t, encoder_hidden_states=torch.cat([uncond, text]), cross_attention_kwargs=plain).sample
        e_u, e_c = e.chunk(2)
        x0 = reverse_step_pred_x0(model, e_u + w_tar * (e_c - e_u), t, xg)
        corr = (e_c - e_u).detach()
        # image by image: each loss is its own decoder / encoder call, so a batch row has the value of a single run
        loss = sum(torch.linalg.norm(encs[i].get_gram_matrix_residual(model.vae.decode(1 / 0.18215 * x0[i:i + 1]).sample))
                   for i in range(n))
        g = torch.autograd.grad(outputs=loss, inputs=xg)[0].detach()
    # the reference's scalars are Python floats: rms / rms * weight in double, rounded once where it meets the tensor
    rms = lambda v: torch.stack([(v[i] * v[i]).mean().sqrt() for i in range(n)]).double()
    rho = (rms(corr) / rms(g) * weight).float().view(-1, 1, 1, 1)
    return x_prev - rho * g


def ef_p2p(model, image_encoder, xT, etas=1.0, prompts="", cfg_scales=None, prog_bar=False, zs=None, controller=None,
           weight_edit_clip=1.5, is_ddim_inversion=False, per_image=False, fused=None):
    assert len(prompts) >= 2, "for prompt-to-prompt, requires both source and target prompts"
    nested = not isinstance(prompts[0], str)
    if nested and not per_image:
        raise ValueError("one [source, target] pair per image needs per_image=True")
    pairs = [list(p[:2]) for p in prompts] if nested else [list(prompts[:2])]
    n = len(pairs)
    if etas is None:
        etas = 0
    if type(etas) in [int, float]:
        etas = [etas] * model.scheduler.num_inference_steps
    assert len(etas) == model.scheduler.num_inference_steps
    if isinstance(image_encoder, (list, tuple)) and len(image_encoder) != n:
        raise ValueError("one image encoder per image expected")
    dev = model.device
    xT = xT.to(dev)
    if xT.dim() < 4:
        xT = xT.unsqueeze(0)
    if xT.shape[0] != n:
        raise ValueError("one [source, target] pair per image expected")
    zs = zs.to(dev).reshape(zs.shape[0], n, *xT.shape[1:])
    cfg_src, cfg_tar = float(cfg_scales[0]), float(cfg_scales[1])
    # every image's prompts as the reference's batch of two: an embedding has the bits of the single run whatever it is batched with
    per = [encode_text(model, p) for p in pairs]
    text = torch.cat([e[:1] for e in per] + [e[1:] for e in per])
    null = encode_text(model, [""] * 2)
    uncond = torch.cat([null[:1]] * n + [null[1:]] * n)
    engine = None
    if _is_hip(model) and fused is not False:
        from ..engine import HEditEngine
        engine = HEditEngine(model)
    steps = zs.shape[0]
    xt = torch.cat([xT, xT])                    # kind-major like the engine's rows: [source] * n, [target] * n
    for i, t in enumerate(list(model.scheduler.timesteps[-steps:])):
        idx = steps - 1 - i
        z = zs[idx]
        with torch.no_grad():
            e = model.unet(torch.cat([xt] * 2), t, encoder_hidden_states=torch.cat([uncond, text])).sample      # the P2P pass
            e_u, e_c = e.chunk(2)
            e_src = e_u[:n] + cfg_src * (e_c[:n] - e_u[:n])
            e_tar = e_u[n:] + cfg_tar * (e_c[n:] - e_u[n:])
            x_src = reverse_step(model, e_src, t, xt[:n], eta=etas[idx], variance_noise=z, is_ddim_inversion=is_ddim_inversion)
            x_tar = reverse_step(model, e_tar, t, xt[n:], eta=0 if is_ddim_inversion else etas[idx], variance_noise=z,
                                 is_ddim_inversion=is_ddim_inversion)
            x_tar = ef_style_update(model, image_encoder, xt[n:], x_tar, uncond[n:], text[n:], t, cfg_tar, weight_edit_clip,
                                    fused=fused, engine=engine)
            xt = torch.cat([x_src, x_tar])
            if controller is not None:
                xt = controller.step_callback(xt)
    return xt[n:], xt[:n]
