#!/usr/bin/env python3
"""The comparison editors of the reference's tables on the HIP path: Edit Friendly (EF), PnP Inversion (PnP-Inv) and
negative-prompt inversion (NP) -- the modes of ``text-guided/main_p2p.py``, ``main_masactrl.py`` and
``main_plugnplay.py`` that need no gradient through the UNet, in one driver:

    mode               inversion                         loop (hedit.inversion)        family
    ef                 DDPM, --eta 1                     ef_wo_p2p                     p2p
    ef_p2p             DDPM, --eta 1                     ef_or_pnp_inv_w_p2p           p2p
    pnp_inv_p2p        DDIM, --eta 0                     ef_or_pnp_inv_w_p2p           p2p
    ef_masactrl        DDPM, --eta 1, source prompt ""   ef_or_pnp_inv_w_masactrl      masactrl
    pnp_inv_masactrl   DDIM, --eta 0, source prompt ""   ef_or_pnp_inv_w_masactrl      masactrl
    np_pnp             DDIM, --eta 0                     negative_prompt_pnp           pnp

Dataset format (PIE-Bench mapping file), image loading, controller / editor / injection set-up and the output
sub-directory follow the reference driver of the mode's family (main_p2p.py:102-103,132,139-146,187-211,249-255;
main_masactrl.py:121-122,149,156-218; main_plugnplay.py:117-118,148,155-225); flags that only appear in that name are
accepted.  Two things differ from the reference on purpose: ``ef`` takes the single tensor ef_wo_p2p returns (the
reference unpacks two values from it, main_p2p.py:250, and stops with ValueError), and ``ef_pnp`` / ``pnp_inv_w_pnp``
are refused (ef_or_pnp_inv_w_pnp asserts etas == 0, pnp_baselines.py:338, while main_plugnplay.py passes 1.0: the
reference modes stop at that assertion).  nmg* and nt_pnp need the gradient of a UNet pass with respect to its input,
which this library does not build, and are refused too; so are, for the same reason, the EF modes of the style and
face drivers (main_edit.py / main_edit_face.py keep refusing them).
Additions as in main_p2p.py: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed``, sharding over ranks under
torch.distributed.run, ``--batch N`` (N entries in lock-step; same bits per image as one at a time)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.driver import BASELINE_MODES as MODES  # noqa: E402
from hedit.engine import HEditEngine  # noqa: E402
from hedit.inversion.masactrl_baselines import ef_or_pnp_inv_w_masactrl  # noqa: E402
from hedit.inversion.p2p_baselines import ef_or_pnp_inv_w_p2p, ef_wo_p2p  # noqa: E402
from hedit.inversion.pnp_baselines import negative_prompt_pnp  # noqa: E402
from hedit.masactrl import MutualSelfAttentionControl, regiter_attention_editor_diffusers  # noqa: E402
from hedit.p2p.ptp_classes import AttentionStore, ControllerBatch  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402

_NEEDS_GRADIENT = ("nmg", "nmg_p2p", "nmg_pnp", "nt_pnp")
_REFERENCE_ASSERTS = ("ef_pnp", "pnp_inv_w_pnp")


def build_parser():
    return DR.comparison_parser("./results/baselines", "ef_p2p", 1.0, MODES)


def edit_group(args, model, entries, scale, size, device):
    """n entries [(key, item, image_path, save_path)] in lock-step: VAE encode, inversion, the mode's loop, VAE decode.
    One entry goes through the reference-signature function of the mode, several through the engine's lock-step
    loops (one controller per image in a ControllerBatch; the MasaCtrl editor and the injection plan cover n images)."""
    eng = HEditEngine(model)
    family, _ = MODES[args.mode]
    n = len(entries)
    is_ddim_inversion = args.eta == 0
    DR.set_scheduler(model, args.num_diffusion_steps, is_ddim_inversion)
    after = args.num_diffusion_steps - args.skip
    tar_p = [DR.clean(item["editing_prompt"]) for _, item, _, _ in entries]
    # MasaCtrl runs without the source prompt (main_masactrl.py:178)
    src_p = [""] * n if family == "masactrl" else [DR.clean(item["original_prompt"]) for _, item, _, _ in entries]
    w0 = DR.encode_images(model, entries, scale, size, device, family)
    zs, wts, eta = DR.invert(args, model, w0, src_p, eng)
    xT, zs = wts[after].contiguous(), zs[:after].contiguous()
    cfg = [args.cfg_src, args.cfg_tar]
    pairs = [[a, b] for a, b in zip(src_p, tar_p)]

    if family == "p2p":
        if args.mode == "ef":
            controller = AttentionStore()
        else:
            # always the Refine controller, equalizer 2.0 (main_p2p.py:187-188, 200-201)
            ctrls = [DR.p2p_controller(args, model, item, after) for _, item, _, _ in entries]
            controller = ctrls[0] if n == 1 else ControllerBatch(ctrls)
        register_attention_control(model, controller)
        if args.mode == "ef":
            if n == 1:
                # ONE tensor: the reference function returns the edited latent alone (p2p_baselines.py:95)
                edited = ef_wo_p2p(model, xT=xT, etas=eta, prompts=[tar_p[0]], cfg_scales=[args.cfg_tar], prog_bar=True,
                                   zs=zs[:, 0], controller=controller, is_ddim_inversion=is_ddim_inversion)
            else:
                edited, _ = eng.run_direct(xT, zs, [[t] for t in tar_p], [args.cfg_tar], controller, eta=eta, after_skip_steps=after,
                                           ddim_inv=is_ddim_inversion, control=False)
        elif n == 1:
            edited, _ = ef_or_pnp_inv_w_p2p(model, xT=xT, etas=eta, prompts=pairs[0], cfg_scales=cfg, prog_bar=True, zs=zs[:, 0],
                                            controller=controller, is_ddim_inversion=is_ddim_inversion)
        else:
            edited, _ = eng.run_direct(xT, zs, pairs, cfg, controller, eta=eta, after_skip_steps=after, ddim_inv=is_ddim_inversion)
    elif family == "masactrl":
        editor = MutualSelfAttentionControl(args.step, args.layer)
        regiter_attention_editor_diffusers(model, editor)
        if n == 1:
            edited, _ = ef_or_pnp_inv_w_masactrl(model, xT=xT, etas=eta, prompts=pairs[0], cfg_scales=cfg, prog_bar=True, zs=zs[:, 0],
                                                 is_ddim_inversion=is_ddim_inversion)
        else:
            edited, _ = eng.run_direct(xT, zs, pairs, cfg, editor, eta=eta, after_skip_steps=after, ddim_inv=is_ddim_inversion)
    else:
        DR.register_pnp(model, after, args.pnp_f_t, args.pnp_attn_t)
        if n == 1:
            edited, _ = negative_prompt_pnp(model, xT=xT, etas=0.0, prompts=pairs[0], cfg_scales=cfg, prog_bar=True, zs=zs[:, 0])
        else:
            edited, _ = eng.run_direct_pnp(xT, None, pairs, [args.cfg_tar, args.cfg_tar], eta=0.0, after_skip_steps=after,
                                           ddim_inv=False, uncond="src")

    out = DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)
    model.unet.zero_grad()
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode in _NEEDS_GRADIENT:
        raise NotImplementedError(f"mode {args.mode}: needs the gradient of a UNet pass with respect to its input (noise-map "
                                  "guidance / null-text optimisation), which this driver does not build; the nmg modes run in main_nmg.py, nt_pnp in main_nt.py")
    if args.mode in _REFERENCE_ASSERTS:
        raise NotImplementedError(f"mode {args.mode}: the reference's ef_or_pnp_inv_w_pnp asserts etas == 0 while its driver passes "
                                  "1.0, so the reference mode cannot run as shipped; the function is in hedit.inversion.pnp_baselines")
    if args.mode not in MODES:
        raise NotImplementedError(f"mode {args.mode}: this driver runs {', '.join(MODES)}; the h-Edit modes have their own drivers")
    family, want_eta = MODES[args.mode]
    assert args.eta == want_eta, f"eta should be {want_eta} for {args.mode}"
    print(f'Arguments: {args}')
    tail = '_' if args.mode == "ef" else DR.family_tail(args, family)      # (ef: main_p2p.py:102 names --xa / --sa for *_p2p only)
    return DR.run_pie_bench(args, tail, edit_group, family=family)


if __name__ == "__main__":
    main()
