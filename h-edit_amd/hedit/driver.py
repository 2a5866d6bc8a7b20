"""What the text-guided editing drivers (h-edit_amd/main_*.py) share: the reference's flag block and this build's
additions, image / model loading, the run's start-up, the per-group steps every ``edit_group`` takes (scheduler set-up,
inversion, Plug-and-Play registration, saving) and the loop over lock-step groups.  A driver keeps what is its own: the
docstring, the flags only it has, its mode table and refusals, and its ``edit_group``.

One entry shape for all drivers: ``(key, item, image_path, save_path)``; ``item`` has ``original_prompt``,
``editing_prompt`` and ``blended_word`` as in the PIE-Bench mapping file."""
import argparse
import calendar
import collections
import json
import os
import time

import numpy as np
import torch

from . import dist as D
from .engine import HEditEngine
from .inversion.ddim_inversion import ddim_inversion
from .inversion.ddpm_inversion import inversion_forward_process_ddpm
from .p2p.ptp_classes import load_512
from .p2p.ptp_controller_utils import make_controller
from .pipeline import HEditPipeline
from .plug_n_play import register_attention_control_efficient, register_conv_control_efficient
from .scheduler import DDIMScheduler
from .text import prescan_prompts
from .utils import image_grid

# the comparison drivers' mode tables (their refusal messages name the driver that runs a mode)
BASELINE_MODES = {"ef": ("p2p", 1.0), "ef_p2p": ("p2p", 1.0), "pnp_inv_p2p": ("p2p", 0.0),       # mode -> (family, eta it needs)
                  "ef_masactrl": ("masactrl", 1.0), "pnp_inv_masactrl": ("masactrl", 0.0), "np_pnp": ("pnp", 0.0)}
NMG_MODES = {"nmg": "p2p", "nmg_p2p": "p2p", "nmg_pnp": "pnp"}      # mode -> family
NT_MODES = {"nt_pnp": "pnp"}


# ------------------------------------------------------------------------------------------ flags
def add_reference_flags(p, output_path, mode, eta, mode_help, data_path="./PIE_Bench_Data", categories=True):
    """the flag block the reference's text-guided drivers share (main_p2p.py:38-62), with the driver's defaults"""
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument('--data_path', type=str, default=data_path)
    p.add_argument('--output_path', type=str, default=output_path)
    if categories:
        p.add_argument('--edit_category_list', nargs='+', type=str, default=[str(i) for i in range(10)])
    p.add_argument("--mode", default=mode, help=mode_help)
    p.add_argument("--num_diffusion_steps", type=int, default=50)
    p.add_argument("--skip", type=int, default=0)
    p.add_argument("--eta", type=float, default=eta)
    p.add_argument("--cfg_src", type=float, default=1.0)
    p.add_argument("--cfg_src_edit", type=float, default=5.0)
    p.add_argument("--cfg_tar", type=float, default=7.5)
    p.add_argument("--implicit", action='store_true', help="Use implicit form of h-Edit")
    p.add_argument("--optimization_steps", type=int, default=1)
    p.add_argument("--weight_reconstruction", type=float, default=0.1)


def add_build_flags(p):
    """the additions of this build"""
    p.add_argument("--model_path", type=str, default=None, help="local SD-1.x checkpoint directory (diffusers layout)")
    p.add_argument("--random_init", action="store_true", help="synthetic SD-1.x-shaped weights (no checkpoint)")
    p.add_argument("--tiny", action="store_true", help="with --random_init: the small test configuration")
    # opt-in, and absent from the namespace unless given (the parsed defaults stay the reference CLI + the additions above)
    p.add_argument("--native_text", action="store_true", default=argparse.SUPPRESS,
                   help="prompts through the native CLIP text encoder (csrc/text.hip), one call per lock-step group")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch", type=int, default=1, help="dataset entries edited in lock-step per pass (batched engine)")


def add_family_flags(p, *families):
    """the flags of a controller family: p2p (--xa / --sa), masactrl (--layer / --step), pnp (--pnp_f_t / --pnp_attn_t)"""
    if "p2p" in families:
        p.add_argument("--xa", type=float, default=0.4)
        p.add_argument("--sa", type=float, default=0.35)
    if "masactrl" in families:
        p.add_argument("--layer", type=int, default=10)
        p.add_argument("--step", type=int, default=4)
    if "pnp" in families:
        p.add_argument("--pnp_f_t", type=float, default=0.45)
        p.add_argument("--pnp_attn_t", type=float, default=0.35)


def comparison_parser(output_path, mode, eta, modes):
    """the parser of a comparison driver (main_baselines.py, main_nmg.py, main_nt.py): one driver covers modes of all three
    reference drivers, so it takes the flags of all three families.  --cfg_src_edit, --implicit, --optimization_steps and
    --weight_reconstruction only name the output directory there."""
    p = argparse.ArgumentParser()
    add_reference_flags(p, output_path, mode, eta, "modes: " + ", ".join(modes))
    add_family_flags(p, "p2p", "masactrl", "pnp")
    add_build_flags(p)
    return p


# ------------------------------------------------------------------------------------------ loading
def clean(s):
    """a dataset prompt without the square brackets around its edited words"""
    return s.replace("[", "").replace("]", "")


def load_image(image_path, device, size=512):
    """main_masactrl.py:39-44 and its twin in main_plugnplay.py: RGB uint8 -> [-1, 1], nearest resize to size x size
    (F.interpolate's default)."""
    from PIL import Image
    a = torch.from_numpy(np.asarray(Image.open(image_path).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1)
    image = a[:3].unsqueeze(0).float() / 127.5 - 1.
    return torch.nn.functional.interpolate(image, (size, size)).to(device)


def load_512_sized(image_path, device, size):
    """the P2P family's load_512 (main_p2p.py:132), then bilinear to size x size (the tiny test configuration works at a
    smaller resolution)"""
    x0 = load_512(image_path, 0, 0, 0, 0, device)
    if x0.shape[-1] != size:
        x0 = torch.nn.functional.interpolate(x0, size=(size, size), mode="bilinear", align_corners=False)
    return x0


def encode_images(model, entries, scale, size, device, family):
    """the entries' images as scaled fp32 latents (n, C, H, W): load_512 and the posterior's mode for the P2P family,
    load_image and its mean for MasaCtrl / Plug-and-Play, as the reference driver of the family does"""
    if family == "p2p":
        return (model.vae.encode(torch.cat([load_512_sized(e[2], device, size) for e in entries])).latent_dist.mode() * scale).float()
    return (model.vae.encode(torch.cat([load_image(e[2], device, size) for e in entries])).latent_dist.mean * scale).float()


def load_model(args, device, family="p2p"):
    """the pipeline --model_path / --random_init / --tiny ask for.  family="pnp": with --tiny the four-level toy UNet
    (the Plug-and-Play injection indexes up_blocks[1..3] with attention) instead of TINY_CONFIG.  ``args.unet_grad``, where a
    driver sets it, builds the UNet with a gradient pass."""
    kw = dict(device=device, native_text=getattr(args, "native_text", False), grad=getattr(args, "unet_grad", False))
    if args.random_init and args.tiny:
        from .unet import TINY_CONFIG
        from .vae import TINY_VAE_CONFIG
        ucfg, vcfg = TINY_CONFIG, dict(TINY_VAE_CONFIG)
        if family == "pnp":
            ucfg = dict(in_channels=4, out_channels=4, sample_size=64, block_out_channels=(64, 64, 128, 128),
                        down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",),
                        up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3, layers_per_block=2,
                        cross_attention_dim=64, attention_head_dim=2, norm_num_groups=32)
            vcfg.update(block_out_channels=(64, 64, 128))                 # f = 4: 256 x 256 images
        else:
            vcfg.update(block_out_channels=(64, 64, 128, 128))          # f = 8 like SD
        return HEditPipeline.from_random(ucfg, seed=args.seed, text_layers=2, vae_config=vcfg, **kw)
    if args.random_init:
        return HEditPipeline.from_random(seed=args.seed, with_vae=True, **kw)
    if not args.model_path:
        raise SystemExit("give --model_path DIR (local diffusers-layout checkpoint) or --random_init")
    return HEditPipeline.from_pretrained(args.model_path, **kw)


# ------------------------------------------------------------------------------------------ run set-up
Run = collections.namedtuple("Run", "rank world device full_data time_stamp model scale size")


def read_mapping_file(data_path):
    with open(os.path.join(data_path, 'mapping_file.json')) as f:
        return json.load(f)


def start_run(args, read_dataset, family="p2p",
              no_vae="the checkpoint has no vae/ sub-folder: images cannot be encoded / decoded"):
    """A run's start-up: rank / device, the process group, the dataset (read_dataset()), the time stamp of the output
    directory, the model, the stand-in tokenizer's vocabulary, the no-VAE refusal, scale and image size."""
    rank, world, local_rank = D.env_rank_world()
    device = f"cuda:{local_rank if world > 1 else args.device_num}"
    torch.cuda.set_device(device)
    D.init_from_env(device)      # several ranks: RCCL group; rank 0 reads the checkpoints and broadcasts them
    full_data = read_dataset()
    time_stamp = calendar.timegm(time.gmtime())
    model = load_model(args, device, family)
    # (stand-in tokenizer only: word ids independent of order / shard)
    prescan_prompts(model.tokenizer, full_data.values() if isinstance(full_data, dict) else full_data)
    if model.vae is None:
        raise SystemExit(no_vae)
    return Run(rank, world, device, full_data, time_stamp, model, model.vae.config["scaling_factor"],
               model.unet.sample_size * model.vae.factor)


def family_tail(args, family):
    """the end of the output sub-directory's name, as the reference driver of the family writes it"""
    if family == "p2p":
        return f'_xa_{args.xa}_sa{args.sa}_'
    if family == "masactrl":
        return f'_step_{args.step}_layer_{args.layer}_'
    return f'_f_t_{args.pnp_f_t}_attn_t_{args.pnp_attn_t}_'


def out_subdir(args, time_stamp, tail, weight=None):
    """mode_total_steps_..._time_<stamp><tail> (main_p2p.py:76-103).  weight: (label, value) of the one field the style
    driver names differently, ("w_rec", --weight_reconstruction) unless given."""
    label, value = weight or ("w_rec", args.weight_reconstruction)
    weight_string = (f'implicit_{args.implicit}_eta_{args.eta}_src_orig_{args.cfg_src}_src_edit_{args.cfg_src_edit}'
                     f'_tar_scale_{args.cfg_tar}_{label}_{value}_n_opts_{args.optimization_steps}'
                     f'_time_{time_stamp}')
    return args.mode + '_total_steps_' + str(args.num_diffusion_steps) + '_skip_' + str(args.skip) + '_' + weight_string + tail


def pie_entries(args, full_data):
    """[(key, item, image_path)] of a PIE-Bench mapping file, the categories of --edit_category_list only"""
    return [(k, item, os.path.join(f"{args.data_path}/annotation_images", item["image_path"]))
            for k, item in full_data.items() if item["editing_type_id"] in args.edit_category_list]


def run_groups(args, run, todo, root, sub, edit_group, **kw):
    """This rank's shard of todo = [(key, item, image_path)], in groups of --batch through edit_group(args, model, entries,
    scale, size, device, **kw); an image is saved where it was read, with root replaced by <output_path>/<sub>.
    -> the written paths."""
    mine = D.shard(len(todo), run.rank, run.world)
    step = max(1, args.batch)
    written = []
    for lo in range(0, len(mine), step):
        entries = [todo[i] + (todo[i][2].replace(root, os.path.join(args.output_path, sub)),) for i in mine[lo:lo + step]]
        written += edit_group(args, run.model, entries, run.scale, run.size, run.device, **kw)
    print(f"rank {run.rank}/{run.world}: wrote {len(written)} image(s)")
    return written


def run_pie_bench(args, tail, edit_group, family="p2p"):
    """the whole run of a driver over a PIE-Bench mapping file, after its own checks of the mode -> the written paths"""
    run = start_run(args, lambda: read_mapping_file(args.data_path), family)
    return run_groups(args, run, pie_entries(args, run.full_data), args.data_path, out_subdir(args, run.time_stamp, tail),
                      edit_group)


# ------------------------------------------------------------------------------------------ per-group steps
def set_scheduler(model, steps, ddim):
    """main_p2p.py:139-146: explicit SD betas for DDIM inversion, the checkpoint's scheduler otherwise"""
    if ddim:
        model.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                        clip_sample=False, set_alpha_to_one=False)
    model.scheduler.config.timestep_spacing = "leading"
    model.scheduler.set_timesteps(steps)


def lock_step_engine(model, n):
    """the batched engine for a group of several entries; None for one, which the h-Edit drivers send through the
    reference-signature functions"""
    return HEditEngine(model) if n > 1 else None


def invert(args, model, w0, src, engine=None):
    """--eta 0: DDIM inversion, and the loop runs at eta 1 (the source row replays the stored corrections u_t^orig,
    main_p2p.py:165); 0 < --eta <= 1: edit-friendly DDPM inversion.  engine: a HEditEngine inverts the n images of w0 in
    lock-step (src: n prompts); without one the reference-signature functions invert one image (src: its prompt).
    -> (zs, wts, the loop's eta)"""
    eta = args.eta
    if eta == 0:
        _, zs, wts = engine.ddim_inversion(w0, src, args.cfg_src) if engine else ddim_inversion(model, w0, src, args.cfg_src)
        return zs, wts, 1.0
    if not 0 < eta <= 1:
        raise SystemExit("Warning: out of range for eta")
    if engine:
        zs, wts = engine.ddpm_inversion(w0, src, eta=eta, cfg_src=args.cfg_src)
    else:
        _, zs, wts, _ = inversion_forward_process_ddpm(model, w0, etas=eta, prompt=src, cfg_scale_src=args.cfg_src,
                                                       num_inference_steps=args.num_diffusion_steps)
    return zs, wts, eta


def p2p_controller(args, model, item, num_steps, replace=False, eq_value=2.0, local_blend=True, eq_extra=None):
    """the P2P controller of one entry (main_p2p.py:187-211): Replace or Refine, local blend on the dataset's blended
    words, its second word re-weighted by eq_value, eq_extra = further equalizer words merged behind it"""
    bw = item["blended_word"].split(" ") if item["blended_word"] != "" else []
    eq_params = {"words": (bw[1],), "values": (eq_value,)} if len(bw) else None
    if eq_extra is not None:
        eq_params = eq_extra if eq_params is None else {"words": eq_params["words"] + eq_extra["words"],
                                                        "values": eq_params["values"] + eq_extra["values"]}
    return make_controller(prompts=[clean(item["original_prompt"]), clean(item["editing_prompt"])], is_replace_controller=replace,
                           cross_replace_steps=args.xa, self_replace_steps=args.sa,
                           blend_word=((bw[0],), (bw[1],)) if len(bw) and local_blend else None, equilizer_params=eq_params,
                           num_steps=num_steps, tokenizer=model.tokenizer, device=model.device)


def register_pnp(model, after, f_t, attn_t):
    """main_plugnplay.py:197-206: inject q, k for the first int(after * attn_t) steps, features for int(after * f_t)"""
    pnp_f_t, pnp_attn_t = int(after * f_t), int(after * attn_t)
    register_attention_control_efficient(model, model.scheduler.timesteps[:pnp_attn_t] if pnp_attn_t >= 0 else [])
    register_conv_control_efficient(model, model.scheduler.timesteps[:pnp_f_t] if pnp_f_t >= 0 else [])


def save_group(x0_dec, entries):
    """image i of the decoded batch to entry i's save_path -> the paths"""
    out = []
    for i, entry in enumerate(entries):
        os.makedirs(os.path.dirname(entry[3]), exist_ok=True)
        image_grid(x0_dec[i:i + 1]).save(entry[3])
        out.append(entry[3])
    return out
