#!/usr/bin/env python3
"""Null-text inversion with Plug-and-Play (``nt_pnp``), the comparison editor of the reference's text-guided tables that
optimises the unconditional embedding, on the HIP path: hedit.inversion.pnp_baselines.nulltext_pnp over a
``UNet2DConditionModel(grad="context")``, whose backward is the executor's context-gradient pass
(hedit_unet_forward_keep / hedit_unet_backward_ctx).

    mode       inversion        loop            pass under                      family
    nt_pnp     DDIM, --eta 0    nulltext_pnp    the Plug-and-Play injection     pnp

This is main_plugnplay.py:219-221: the DDIM inversion's latents are the ground truth of the inner optimisation, ten Adam
updates per step at the most (``optimization_steps=10`` is what the reference driver passes whatever ``--optimization_steps``
says; that argument only names the output directory, as there).  Dataset format, image loading, injection set-up and the
output sub-directory follow the reference driver, through hedit/driver.py like main_nmg.py.  Every other mode is refused with the
driver that runs it.  Additions as in main_p2p.py: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed``, sharding
over ranks under torch.distributed.run, ``--batch N`` (N entries in lock-step: one embedding, one optimiser and one loss per
image, the same bits per image as one at a time)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.driver import BASELINE_MODES, NMG_MODES, NT_MODES as MODES  # noqa: E402
from hedit.engine import HEditEngine  # noqa: E402
from hedit.inversion.pnp_baselines import nulltext_pnp  # noqa: E402

NT = dict(optimization_steps=10)   # main_plugnplay.py:221


def build_parser():
    return DR.comparison_parser("./results/nt", "nt_pnp", 0.0, MODES)


def edit_group(args, model, entries, scale, size, device):
    """n entries [(key, item, image_path, save_path)] in lock-step: VAE encode, DDIM inversion (its latents are the ground
    truth of the inner optimisation), nulltext_pnp, VAE decode."""
    n = len(entries)
    DR.set_scheduler(model, args.num_diffusion_steps, True)
    after = args.num_diffusion_steps - args.skip
    pairs = [[DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])] for _, item, _, _ in entries]
    w0 = DR.encode_images(model, entries, scale, size, device, "pnp")
    zs, wts, _ = DR.invert(args, model, w0, [p[0] for p in pairs], HEditEngine(model))      # wts (T + 1, n, C, H, W), x_0 first
    DR.register_pnp(model, after, args.pnp_f_t, args.pnp_attn_t)
    edited, _ = nulltext_pnp(model, xT=wts[after].contiguous(), xT_ori=wts[:after + 1], etas=0.0, prompts=pairs[0] if n == 1 else pairs,
                             cfg_scales=[args.cfg_src, args.cfg_tar], prog_bar=True, zs=zs[:after], per_image=True, **NT)
    out = DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)
    model.unet.zero_grad()
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode not in MODES:
        where = ("main_nmg.py" if args.mode in NMG_MODES else "main_baselines.py" if args.mode in BASELINE_MODES else
                 "the h-Edit drivers")
        raise NotImplementedError(f"mode {args.mode}: this driver runs {', '.join(MODES)}; see {where}")
    assert args.eta == 0.0, f"eta should be 0.0 for {args.mode}"
    print(f'Arguments: {args}')
    args.unet_grad = "context"         # the loader builds the UNet with its context-gradient weights
    return DR.run_pie_bench(args, DR.family_tail(args, "pnp"), edit_group, family="pnp")


if __name__ == "__main__":
    main()
