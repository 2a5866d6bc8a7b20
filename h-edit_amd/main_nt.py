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
output sub-directory follow the reference driver, through main_nmg.py's machinery.  Every other mode is refused with the
driver that runs it.  Additions as in main_p2p.py: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed``, sharding
over ranks under torch.distributed.run, ``--batch N`` (N entries in lock-step: one embedding, one optimiser and one loss per
image, the same bits per image as one at a time)."""
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
from hedit.inversion.pnp_baselines import nulltext_pnp  # noqa: E402
from hedit.plug_n_play import register_attention_control_efficient, register_conv_control_efficient  # noqa: E402
from hedit.scheduler import DDIMScheduler  # noqa: E402
from hedit.text import prescan_prompts  # noqa: E402
from hedit.utils import image_grid  # noqa: E402
from main_baselines import MODES as BASELINE_MODES, _clean, build_parser as baseline_parser  # noqa: E402
from main_masactrl import load_image  # noqa: E402
from main_nmg import MODES as NMG_MODES  # noqa: E402
from main_plugnplay import load_pnp_model  # noqa: E402

MODES = {"nt_pnp": "pnp"}          # mode -> family
NT = dict(optimization_steps=10)   # main_plugnplay.py:221


def build_parser():
    p = baseline_parser()
    p.set_defaults(mode="nt_pnp", eta=0.0, output_path="./results/nt")
    return p


def edit_group(args, model, entries, scale, size, device):
    """n entries [(item, image_path, save_path)] in lock-step: VAE encode, DDIM inversion (its latents are the ground truth
    of the inner optimisation), nulltext_pnp, VAE decode."""
    eng = HEditEngine(model)
    n = len(entries)
    model.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                                    set_alpha_to_one=False)
    model.scheduler.config.timestep_spacing = "leading"
    model.scheduler.set_timesteps(args.num_diffusion_steps)
    after = args.num_diffusion_steps - args.skip
    src_p = [_clean(item["original_prompt"]) for item, _, _ in entries]
    tar_p = [_clean(item["editing_prompt"]) for item, _, _ in entries]
    w0 = (model.vae.encode(torch.cat([load_image(ip, device, size) for _, ip, _ in entries])).latent_dist.mean * scale).float()
    _, zs, wts = eng.ddim_inversion(w0, src_p, args.cfg_src)              # wts (T + 1, n, C, H, W), x_0 first
    pairs = [[a, b] for a, b in zip(src_p, tar_p)]
    pnp_f_t, pnp_attn_t = int(after * args.pnp_f_t), int(after * args.pnp_attn_t)
    register_attention_control_efficient(model, model.scheduler.timesteps[:pnp_attn_t] if pnp_attn_t >= 0 else [])
    register_conv_control_efficient(model, model.scheduler.timesteps[:pnp_f_t] if pnp_f_t >= 0 else [])
    edited, _ = nulltext_pnp(model, xT=wts[after].contiguous(), xT_ori=wts[:after + 1], etas=0.0, prompts=pairs[0] if n == 1 else pairs,
                             cfg_scales=[args.cfg_src, args.cfg_tar], prog_bar=True, zs=zs[:after], per_image=True, **NT)
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
    if args.mode not in MODES:
        where = ("main_nmg.py" if args.mode in NMG_MODES else "main_baselines.py" if args.mode in BASELINE_MODES else
                 "the h-Edit drivers")
        raise NotImplementedError(f"mode {args.mode}: this driver runs {', '.join(MODES)}; see {where}")
    assert args.eta == 0.0, f"eta should be 0.0 for {args.mode}"
    print(f'Arguments: {args}')
    args.unet_grad = "context"         # the loaders build the UNet with its context-gradient weights

    rank, world, local_rank = D.env_rank_world()
    device = f"cuda:{local_rank if world > 1 else args.device_num}"
    torch.cuda.set_device(device)
    D.init_from_env(device)
    data_path, output_path = args.data_path, args.output_path
    with open(os.path.join(data_path, 'mapping_file.json')) as f:
        full_data = json.load(f)
    time_stamp = calendar.timegm(time.gmtime())
    weight_string = (f'implicit_{args.implicit}_eta_{args.eta}_src_orig_{args.cfg_src}_src_edit_{args.cfg_src_edit}'
                     f'_tar_scale_{args.cfg_tar}_w_rec_{args.weight_reconstruction}_n_opts_{args.optimization_steps}'
                     f'_time_{time_stamp}')
    sub = (args.mode + '_total_steps_' + str(args.num_diffusion_steps) + '_skip_' + str(args.skip) + '_' + weight_string +
           f'_f_t_{args.pnp_f_t}_attn_t_{args.pnp_attn_t}_')

    model = load_pnp_model(args, device)
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
