"""Edit Friendly for face swapping -- drop-in for the reference's face-swapping/inversion/ef.py:7-113, the comparison
column of the face task.  Same signature, defaults and return value.  Unlike h-Edit-R (h_edit_R.py) the rewards are
differentiated w.r.t. ``xt`` THROUGH the eps-network (ef.py:64-66, :89-108), so ``model`` must be differentiable in
its first argument: ``hedit.diffusion.Model(grad=True)`` (the HIP executor's input-gradient pass behind an autograd
node), or any torch callable ``model(x, t_vector)`` -- with a torch module on the CPU the function runs on plain autograd.

The reference's quirks are kept:
  * the eta = 0.5 kernel for x_{t-1} (ef.py:75-79), whatever ``eta`` says (``eta`` only scales the noise term);
  * rho = sqrt(alpha_bar[t]) * weight with alpha_bar at t, not t-1 (:90);
  * the mask multiplies the identity step only (:97-100), the LPIPS step is unmasked (:108);
  * the loop breaks before the last update when tm1 == 0 and returns the ``xt`` of that iteration (:81-82, :114): the
    result is one step short of x_0."""
import torch


def ef(model, lpipsloss, idloss, xT, betas, seq, eta=1.0, zs=None, weight_edit_face=100.0, after_skip_steps=100,
       num_inference_steps=100, soft_face_mask=None, per_image=False):
    """per_image (addition, default off = the reference's arithmetic): as in h_Edit_R -- with n > 1 images in lock-step
    the losses are batch means, so each image's gradient carries a factor 1/n; per_image=True multiplies it back.  Here the
    LOSS is scaled, not the gradient: the cotangent that enters the eps-network's backward is then the single run's, where a
    1/n-scaled one would round differently in 16-bit gradient storage (half's subnormals)."""
    if type(eta) in [int, float]:
        etas = [eta] * num_inference_steps
    else:
        etas = eta
    assert len(etas) == num_inference_steps
    timesteps = seq
    xt = xT.unsqueeze(0) if xT.dim() < 4 else xT
    op = list(timesteps[-after_skip_steps:])
    t_to_idx = {int(v): k for k, v in enumerate(timesteps[-after_skip_steps:])}
    alpha_bar = (1.0 - betas).cumprod(dim=0)
    n = xt.size(0)
    gscale = float(n) if per_image else 1.0
    host_t = getattr(model, "accepts_host_timesteps", False)
    xt = xt.detach().requires_grad_(True)

    for i, t in enumerate(op):
        idx = num_inference_steps - t_to_idx[int(t)] - (num_inference_steps - after_skip_steps + 1)
        z = zs[idx] if zs is not None else None
        with torch.enable_grad():
            t_input = torch.ones(n) * t
            eps_t = model(xt, t_input if host_t else t_input.to(xt.device))
            x0_pred = (xt - (1 - alpha_bar[t]) ** 0.5 * eps_t) / alpha_bar[t] ** 0.5       # Tweedie
        tm1 = op[i + 1] if i < len(op) - 1 else 0
        c1 = (1 - alpha_bar[tm1]).sqrt() * 0.5
        c2 = (1 - alpha_bar[tm1]).sqrt() * ((1 - 0.5 ** 2) ** 0.5)
        x_tm1 = alpha_bar[tm1].sqrt() * x0_pred.detach() + c2 * eps_t.detach()
        if z is not None:
            x_tm1 = x_tm1 + (etas[idx] * c1) * z
        if tm1 == 0:
            break
        rho = alpha_bar[t].sqrt() * weight_edit_face
        with torch.enable_grad():
            if idloss:
                id_loss = idloss.get_cosine_loss(x0_pred)
                g = torch.autograd.grad(outputs=id_loss * gscale if per_image else id_loss, inputs=xt, retain_graph=bool(lpipsloss))[0]
                step = rho * g.detach()
                if soft_face_mask is not None:
                    step = step * soft_face_mask
                x_tm1 = x_tm1 - step
            if lpipsloss:
                lpips_loss = lpipsloss.get_lpips_loss(x0_pred)
                g = torch.autograd.grad(outputs=lpips_loss * gscale if per_image else lpips_loss, inputs=xt)[0]
                x_tm1 = x_tm1 - rho * g.detach()
        xt = x_tm1.detach().requires_grad_(True)
    return xt
