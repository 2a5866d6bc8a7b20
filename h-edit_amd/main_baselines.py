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
import argparse
import calendar
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import dist as D  # noqa: E402
from hedit.engine import HEditEngine  # noqa: E402
from hedit.inversion.masactrl_baselines import ef_or_pnp_inv_w_masactrl  # noqa: E402
from hedit.inversion.p2p_baselines import ef_or_pnp_inv_w_p2p, ef_wo_p2p  # noqa: E402
from hedit.inversion.pnp_baselines import negative_prompt_pnp  # noqa: E402
from hedit.masactrl import MutualSelfAttentionControl, regiter_attention_editor_diffusers  # noqa: E402
from hedit.p2p.ptp_classes import AttentionStore, ControllerBatch, load_512  # noqa: E402
from hedit.p2p.ptp_controller_utils import make_controller  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402
from hedit.plug_n_play import register_attention_control_efficient, register_conv_control_efficient  # noqa: E402
from hedit.scheduler import DDIMScheduler  # noqa: E402
from hedit.text import prescan_prompts  # noqa: E402
from hedit.utils import image_grid  # noqa: E402
from main_masactrl import load_image  # noqa: E402
from main_p2p import load_model  # noqa: E402
from main_plugnplay import load_pnp_model  # noqa: E402

# mode -> (family, eta the mode needs)
MODES = {"ef": ("p2p", 1.0), "ef_p2p": ("p2p", 1.0), "pnp_inv_p2p": ("p2p", 0.0),
         "ef_masactrl": ("masactrl", 1.0), "pnp_inv_masactrl": ("masactrl", 0.0), "np_pnp": ("pnp", 0.0)}
_NEEDS_GRADIENT = ("nmg", "nmg_p2p", "nmg_pnp", "nt_pnp")
_REFERENCE_ASSERTS = ("ef_pnp", "pnp_inv_w_pnp")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument('--data_path', type=str, default="./PIE_Bench_Data")
    p.add_argument('--output_path', type=str, default="./results/baselines")
    p.add_argument('--edit_category_list', nargs='+', type=str, default=[str(i) for i in range(10)])
    p.add_argument("--mode", default="ef_p2p", help="modes: " + ", ".join(MODES))
    p.add_argument("--num_diffusion_steps", type=int, default=50)
    p.add_argument("--skip", type=int, default=0)
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--cfg_src", type=float, default=1.0)
    p.add_argument("--cfg_src_edit", type=float, default=5.0)       # (name of the output directory only)
    p.add_argument("--cfg_tar", type=float, default=7.5)
    p.add_argument("--implicit", action='store_true')                # (name only)
    p.add_argument("--optimization_steps", type=int, default=1)     # (name only)
    p.add_argument("--weight_reconstruction", type=float, default=0.1)      # (name only)
    p.add_argument("--xa", type=float, default=0.4)
    p.add_argument("--sa", type=float, default=0.35)
    p.add_argument("--layer", type=int, default=10)
    p.add_argument("--step", type=int, default=4)
    p.add_argument("--pnp_f_t", type=float, default=0.45)
    p.add_argument("--pnp_attn_t", type=float, default=0.35)
    p.add_argument("--model_path", type=str, default=None, help="local SD-1.x checkpoint directory (diffusers layout)")
    p.add_argument("--random_init", action="store_true", help="synthetic SD-1.x-shaped weights (no checkpoint)")
    p.add_argument("--tiny", action="store_true", help="with --random_init: the small test configuration")
    # opt-in, and absent from the namespace unless given (the parsed defaults stay the reference CLI + the additions above)
    p.add_argument("--native_text", action="store_true", default=argparse.SUPPRESS,
                   help="prompts through the native CLIP text encoder (csrc/text.hip), one call per lock-step group")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch", type=int, default=1, help="dataset entries edited in lock-step per pass")
    return p


def _clean(s):
    return s.replace("[", "").replace("]", "")


def edit_group(args, model, entries, scale, size, device):
    """n entries [(item, image_path, save_path)] in lock-step: VAE encode, inversion, the mode's loop, VAE decode.
    One entry goes through the reference-signature function of the mode, several through the engine's lock-step
    loops (one controller per image in a ControllerBatch; the MasaCtrl editor and the injection plan cover n images)."""
    eng = HEditEngine(model)
    family, _ = MODES[args.mode]
    n = len(entries)
    is_ddim_inversion = args.eta == 0
    if is_ddim_inversion:             # explicit SD betas for DDIM inversion, the checkpoint's scheduler otherwise
        model.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                        clip_sample=False, set_alpha_to_one=False)
    model.scheduler.config.timestep_spacing = "leading"
    model.scheduler.set_timesteps(args.num_diffusion_steps)
    T = args.num_diffusion_steps
    after = T - args.skip
    tar_p = [_clean(item["editing_prompt"]) for item, _, _ in entries]
    # MasaCtrl runs without the source prompt (main_masactrl.py:178)
    src_p = [""] * n if family == "masactrl" else [_clean(item["original_prompt"]) for item, _, _ in entries]
    if family == "p2p":
        xs = []
        for _, ip, _ in entries:
            x0 = load_512(ip, 0, 0, 0, 0, device)
            if x0.shape[-1] != size:
                x0 = torch.nn.functional.interpolate(x0, size=(size, size), mode="bilinear", align_corners=False)
            xs.append(x0)
        w0 = (model.vae.encode(torch.cat(xs)).latent_dist.mode() * scale).float()
    else:
        w0 = (model.vae.encode(torch.cat([load_image(ip, device, size) for _, ip, _ in entries])).latent_dist.mean * scale).float()

    if is_ddim_inversion:
        _, zs, wts = eng.ddim_inversion(w0, src_p, args.cfg_src)
        eta = 1.0                     # the source row replays the stored corrections u_t^orig (main_p2p.py:165)
    else:
        zs, wts = eng.ddpm_inversion(w0, src_p, eta=args.eta, cfg_src=args.cfg_src)
        eta = args.eta
    xT, zs = wts[after].contiguous(), zs[:after].contiguous()
    cfg = [args.cfg_src, args.cfg_tar]
    pairs = [[a, b] for a, b in zip(src_p, tar_p)]

    if family == "p2p":
        if args.mode == "ef":
            controller = AttentionStore()
        else:
            ctrls = []
            for item, _, _ in entries:
                bw = item["blended_word"].split(" ") if item["blended_word"] != "" else []
                # always the Refine controller, equalizer 2.0 (main_p2p.py:187-188, 200-201)
                ctrls.append(make_controller(prompts=[_clean(item["original_prompt"]), _clean(item["editing_prompt"])],
                                             is_replace_controller=False, cross_replace_steps=args.xa, self_replace_steps=args.sa,
                                             blend_word=((bw[0],), (bw[1],)) if len(bw) else None,
                                             equilizer_params={"words": (bw[1],), "values": (2.0,)} if len(bw) else None,
                                             num_steps=after, tokenizer=model.tokenizer, device=model.device))
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
        pnp_f_t, pnp_attn_t = int(after * args.pnp_f_t), int(after * args.pnp_attn_t)
        register_attention_control_efficient(model, model.scheduler.timesteps[:pnp_attn_t] if pnp_attn_t >= 0 else [])
        register_conv_control_efficient(model, model.scheduler.timesteps[:pnp_f_t] if pnp_f_t >= 0 else [])
        if n == 1:
            edited, _ = negative_prompt_pnp(model, xT=xT, etas=0.0, prompts=pairs[0], cfg_scales=cfg, prog_bar=True, zs=zs[:, 0])
        else:
            edited, _ = eng.run_direct_pnp(xT, None, pairs, [args.cfg_tar, args.cfg_tar], eta=0.0, after_skip_steps=after,
                                           ddim_inv=False, uncond="src")

    x0_dec = model.vae.decode(1 / scale * edited).sample
    out = []
    for i, (_, _, save_path) in enumerate(entries):
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        image_grid(x0_dec[i:i + 1]).save(save_path)
        out.append(save_path)
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

    rank, world, local_rank = D.env_rank_world()
    device = f"cuda:{local_rank if world > 1 else args.device_num}"
    torch.cuda.set_device(device)
    D.init_from_env(device)
    data_path, output_path = args.data_path, args.output_path
    with open(os.path.join(data_path, 'mapping_file.json')) as f:
        full_data = json.load(f)
    time_stamp = calendar.timegm(time.gmtime())
    if family == "p2p":
        tail = f'_xa_{args.xa}_sa{args.sa}_' if args.mode in ('pnp_inv_p2p', 'ef_p2p') else '_'
    elif family == "masactrl":
        tail = f'_step_{args.step}_layer_{args.layer}_'
    else:
        tail = f'_f_t_{args.pnp_f_t}_attn_t_{args.pnp_attn_t}_'
    weight_string = (f'implicit_{args.implicit}_eta_{args.eta}_src_orig_{args.cfg_src}_src_edit_{args.cfg_src_edit}'
                     f'_tar_scale_{args.cfg_tar}_w_rec_{args.weight_reconstruction}_n_opts_{args.optimization_steps}'
                     f'_time_{time_stamp}')
    sub = args.mode + '_total_steps_' + str(args.num_diffusion_steps) + '_skip_' + str(args.skip) + '_' + weight_string + tail

    model = load_pnp_model(args, device) if family == "pnp" else load_model(args, device)
    prescan_prompts(model.tokenizer, full_data.values())
    if model.vae is None:
        raise SystemExit("the checkpoint has no vae/ sub-folder: images cannot be encoded / decoded")
    scale = model.vae.config["scaling_factor"]
    size = model.unet.sample_size * model.vae.factor
    keys = [k for k, item in full_data.items() if item["editing_type_id"] in args.edit_category_list]
    mine = list(D.shard(len(keys), rank, world))
    written = []
    for lo in range(0, len(mine), max(1, args.batch)):
        entries = []
        for idx in mine[lo:lo + max(1, args.batch)]:
            item = full_data[keys[idx]]
            image_path = os.path.join(f"{data_path}/annotation_images", item["image_path"])
            entries.append((item, image_path, image_path.replace(data_path, os.path.join(output_path, sub))))
        written += edit_group(args, model, entries, scale, size, device)
    print(f"rank {rank}/{world}: wrote {len(written)} image(s)")
    return written


if __name__ == "__main__":
    main()
