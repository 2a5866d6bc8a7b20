"""fp32 restatement of the reference's Edit Friendly face loop (face-swapping/inversion/ef.py:7-113) over any differentiable
callable ``model(x, t_vector)``, PINNED on vectors from running that module (tests/test_host_face_ef.py, g21).  Test
infrastructure, like baseline_ref.py: it lives under tests/ because oracle/ is frozen.

``detach_eps=True`` cuts the UNet Jacobian (the rewards then see xt through the Tweedie map's explicit term only): the
GPU tests use it to show that a comparison is sensitive to the input gradient of the eps-network at all.
``autocast_bf16(model)`` wraps a CPU torch module so that its convolutions / matmuls run on bfloat16 operands: the
yardstick for what 16-bit storage does to the loop."""
import torch


def ef_ref(model, lpipsloss, idloss, xT, betas, seq, eta=1.0, zs=None, weight_edit_face=100.0, after_skip_steps=100,
           num_inference_steps=100, soft_face_mask=None, detach_eps=False, trace=None):
    """trace: optional list that receives the xt each iteration starts from (teacher forcing in failure reports)"""
    etas = [eta] * num_inference_steps
    xt = xT.unsqueeze(0) if xT.dim() < 4 else xT
    op = [int(t) for t in seq[-after_skip_steps:]]
    alpha_bar = (1.0 - betas).cumprod(dim=0)
    n = xt.size(0)
    xt = xt.detach().clone().requires_grad_(True)
    for i, t in enumerate(op):
        idx = num_inference_steps - i - (num_inference_steps - after_skip_steps + 1)
        if trace is not None:
            trace.append(xt.detach().clone())
        with torch.enable_grad():
            eps = model(xt, (torch.ones(n) * t).to(xt.device))
            if detach_eps:
                eps = eps.detach()
            x0 = (xt - (1 - alpha_bar[t]) ** 0.5 * eps) / alpha_bar[t] ** 0.5
        tm1 = op[i + 1] if i < len(op) - 1 else 0
        c1 = (1 - alpha_bar[tm1]).sqrt() * 0.5
        c2 = (1 - alpha_bar[tm1]).sqrt() * ((1 - 0.5 ** 2) ** 0.5)
        x_tm1 = alpha_bar[tm1].sqrt() * x0.detach() + c2 * eps.detach() + (etas[idx] * c1) * zs[idx]
        if tm1 == 0:
            break
        rho = alpha_bar[t].sqrt() * weight_edit_face
        if idloss:
            (g,) = torch.autograd.grad(idloss.get_cosine_loss(x0), xt, retain_graph=True)
            x_tm1 = x_tm1 - rho * g * soft_face_mask if soft_face_mask is not None else x_tm1 - rho * g
        if lpipsloss:
            (g,) = torch.autograd.grad(lpipsloss.get_lpips_loss(x0), xt)
            x_tm1 = x_tm1 - rho * g
        xt = x_tm1.detach().requires_grad_(True)
    return xt


def autocast_bf16(model):
    """the same callable with its convolutions and matrix products on bfloat16 operands (torch.autocast on the CPU),
    fp32 in and out"""
    def run(x, t):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            return model(x, t).float()
    return run
