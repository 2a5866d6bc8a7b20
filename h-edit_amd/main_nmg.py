#!/usr/bin/env python3
"""Noise Map Guidance (NMG), the comparison editor of the reference's text-guided tables that differentiates through the
UNet, on the HIP path: the loops of hedit.inversion (nmg_p2p, nmg_pnp) over a ``UNet2DConditionModel(grad=True)``, whose
backward is the executor's input-gradient pass (hedit_unet_forward_keep / hedit_unet_backward).

    mode       inversion        loop       pass under                        family
    nmg        DDIM, --eta 0    nmg_p2p    nothing (a store nobody reads)    p2p
    nmg_p2p    DDIM, --eta 0    nmg_p2p    the P2P controller                p2p
    nmg_pnp    DDIM, --eta 0    nmg_pnp    the Plug-and-Play injection       pnp

``nmg`` is what the reference dispatches: main_p2p.py:238 tests ``args.mode == 'nmg'``, and since that name does not end
in ``p2p`` the controller is the plain AttentionStore (:187-205), which edits nothing and whose maps nothing reads -- here the
controlled pass of that mode simply runs plain.  ``nmg_p2p`` is the same loop under the P2P controller of make_controller:
what the reference's help text and its output-name rule (main_p2p.py:49, :102) intend, but its dispatch never reaches -- at
that name it raises NotImplementedError (:262).  Running it is a deliberate difference, like ``ef`` in main_baselines.py.
``nmg_pnp`` is main_plugnplay.py:215-218.  guidance_noise_map = 10, grad_scale = 5e3 as the reference passes them.

Dataset format, image loading, controller / injection set-up and the output sub-directory follow the reference driver of the
mode's family, as in main_baselines.py (both on hedit/driver.py); main_baselines.py itself keeps refusing these names.
``nt_pnp`` stays refused here: null-text inversion needs the gradient with respect to the text context, which the
input-gradient pass of ``grad=True`` does not form; it runs in main_nt.py over ``grad="context"``.  Additions as in main_p2p.py: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed``, sharding
over ranks under torch.distributed.run, ``--batch N`` (N entries in lock-step, the L1 mean per image: same bits per image as
one at a time)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.driver import BASELINE_MODES, NMG_MODES as MODES  # noqa: E402
from hedit.engine import HEditEngine  # noqa: E402
from hedit.inversion.p2p_baselines import nmg_p2p  # noqa: E402
from hedit.inversion.pnp_baselines import nmg_pnp  # noqa: E402
from hedit.p2p.ptp_classes import ControllerBatch  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402

NMG = dict(guidance_noise_map=10.0, grad_scale=5e+3)             # main_p2p.py:240, main_plugnplay.py:217


def build_parser():
    return DR.comparison_parser("./results/nmg", "nmg_p2p", 0.0, MODES)


def edit_group(args, model, entries, scale, size, device):
    """n entries [(key, item, image_path, save_path)] in lock-step: VAE encode, DDIM inversion (its latents are the loop's
    ground truth), the mode's loop, VAE decode."""
    family = MODES[args.mode]
    n = len(entries)
    DR.set_scheduler(model, args.num_diffusion_steps, True)
    after = args.num_diffusion_steps - args.skip
    pairs = [[DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])] for _, item, _, _ in entries]
    w0 = DR.encode_images(model, entries, scale, size, device, family)
    zs, wts, _ = DR.invert(args, model, w0, [p[0] for p in pairs], HEditEngine(model))      # wts (T + 1, n, C, H, W), x_0 first
    kw = dict(xT=wts[after].contiguous(), xT_ori=wts[:after + 1], etas=0.0, prompts=pairs[0] if n == 1 else pairs,
              cfg_scales=[args.cfg_src, args.cfg_tar], prog_bar=True, zs=zs[:after], per_image=True, **NMG)      # (one image: the per-image mean is the reference's)

    if family == "p2p":
        controller = None
        if args.mode == "nmg_p2p":
            # always the Refine controller, equalizer 2.0 (main_p2p.py:187-188, 200-201)
            ctrls = [DR.p2p_controller(args, model, item, after) for _, item, _, _ in entries]
            controller = ctrls[0] if n == 1 else ControllerBatch(ctrls)
            register_attention_control(model, controller)
        edited, _ = nmg_p2p(model, controller=controller, **kw)
    else:
        DR.register_pnp(model, after, args.pnp_f_t, args.pnp_attn_t)
        edited, _ = nmg_pnp(model, **kw)

    out = DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)
    model.unet.zero_grad()
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == "nt_pnp":
        raise NotImplementedError("mode nt_pnp: null-text inversion optimises the unconditional embedding, i.e. it needs the gradient "
                                  "with respect to the text context, which the UNet's input-gradient pass of this driver does not "
                                  "form; the mode runs in main_nt.py")
    if args.mode not in MODES:
        where = "main_baselines.py" if args.mode in BASELINE_MODES else "the h-Edit drivers"
        raise NotImplementedError(f"mode {args.mode}: this driver runs {', '.join(MODES)}; see {where}")
    assert args.eta == 0.0, f"eta should be 0.0 for {args.mode}"
    print(f'Arguments: {args}')
    family = MODES[args.mode]
    args.unet_grad = True              # the loader builds the UNet with its input-gradient weights
    tail = '_' if args.mode == "nmg" else DR.family_tail(args, family)
    return DR.run_pie_bench(args, tail, edit_group, family=family)


if __name__ == "__main__":
    main()
