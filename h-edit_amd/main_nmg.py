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
mode's family, as in main_baselines.py, whose machinery this driver uses; main_baselines.py itself keeps refusing these names.
``nt_pnp`` stays refused here: null-text inversion needs the gradient with respect to the text context, which the
input-gradient pass of ``grad=True`` does not form; it runs in main_nt.py over ``grad="context"``.  Additions as in main_p2p.py: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed``, sharding
over ranks under torch.distributed.run, ``--batch N`` (N entries in lock-step, the L1 mean per image: same bits per image as
one at a time)."""
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
from hedit.inversion.p2p_baselines import nmg_p2p  # noqa: E402
from hedit.inversion.pnp_baselines import nmg_pnp  # noqa: E402
from hedit.p2p.ptp_classes import ControllerBatch, load_512  # noqa: E402
from hedit.p2p.ptp_controller_utils import make_controller  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402
from hedit.plug_n_play import register_attention_control_efficient, register_conv_control_efficient  # noqa: E402
from hedit.scheduler import DDIMScheduler  # noqa: E402
from hedit.text import prescan_prompts  # noqa: E402
from hedit.utils import image_grid  # noqa: E402
from main_baselines import MODES as BASELINE_MODES, _clean, build_parser as baseline_parser  # noqa: E402
from main_masactrl import load_image  # noqa: E402
from main_p2p import load_model  # noqa: E402
from main_plugnplay import load_pnp_model  # noqa: E402

MODES = {"nmg": "p2p", "nmg_p2p": "p2p", "nmg_pnp": "pnp"}      # mode -> family
NMG = dict(guidance_noise_map=10.0, grad_scale=5e+3)             # main_p2p.py:240, main_plugnplay.py:217


def build_parser():
    p = baseline_parser()
    p.set_defaults(mode="nmg_p2p", eta=0.0, output_path="./results/nmg")
    return p


def edit_group(args, model, entries, scale, size, device):
    """n entries [(item, image_path, save_path)] in lock-step: VAE encode, DDIM inversion (its latents are the loop's ground
    truth), the mode's loop, VAE decode."""
    eng = HEditEngine(model)
    family = MODES[args.mode]
    n = len(entries)
    model.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                                    set_alpha_to_one=False)
    model.scheduler.config.timestep_spacing = "leading"
    model.scheduler.set_timesteps(args.num_diffusion_steps)
    after = args.num_diffusion_steps - args.skip
    src_p = [_clean(item["original_prompt"]) for item, _, _ in entries]
    tar_p = [_clean(item["editing_prompt"]) for item, _, _ in entries]
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
    _, zs, wts = eng.ddim_inversion(w0, src_p, args.cfg_src)              # wts (T + 1, n, C, H, W), x_0 first
    pairs = [[a, b] for a, b in zip(src_p, tar_p)]
    kw = dict(xT=wts[after].contiguous(), xT_ori=wts[:after + 1], etas=0.0, prompts=pairs[0] if n == 1 else pairs,
              cfg_scales=[args.cfg_src, args.cfg_tar], prog_bar=True, zs=zs[:after], per_image=True, **NMG)      # (one image: the per-image mean is the reference's)

    if family == "p2p":
        controller = None
        if args.mode == "nmg_p2p":
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
        edited, _ = nmg_p2p(model, controller=controller, **kw)
    else:
        pnp_f_t, pnp_attn_t = int(after * args.pnp_f_t), int(after * args.pnp_attn_t)
        register_attention_control_efficient(model, model.scheduler.timesteps[:pnp_attn_t] if pnp_attn_t >= 0 else [])
        register_conv_control_efficient(model, model.scheduler.timesteps[:pnp_f_t] if pnp_f_t >= 0 else [])
        edited, _ = nmg_pnp(model, **kw)

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
    args.unet_grad = True              # the loaders build the UNet with its input-gradient weights

    rank, world, local_rank = D.env_rank_world()
    device = f"cuda:{local_rank if world > 1 else args.device_num}"
    torch.cuda.set_device(device)
    D.init_from_env(device)
    data_path, output_path = args.data_path, args.output_path
    with open(os.path.join(data_path, 'mapping_file.json')) as f:
        full_data = json.load(f)
    time_stamp = calendar.timegm(time.gmtime())
    tail = f'_xa_{args.xa}_sa{args.sa}_' if args.mode == "nmg_p2p" else ('_' if family == "p2p" else f'_f_t_{args.pnp_f_t}_attn_t_{args.pnp_attn_t}_')
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
