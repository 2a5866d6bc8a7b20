#!/usr/bin/env python3
"""Combined text-guided + style editing driver on the HIP path: same flags, dataset format
(``<dataset>/demo.json`` with ``image_path / original_prompt / editing_prompt / blended_word / style``)
and output-path scheme as the reference's ``text-guided-n-style/main_edit.py`` (:33-73 flags,
:91-99 strings, :103-247 loop) for its h-Edit mode (``h_edit_R_p2p``).

Differences, all additive:
  * ``--model_path DIR``: LOCAL Stable-Diffusion checkpoint directory (diffusers layout);
    ``--clip_path FILE``: LOCAL OpenAI CLIP ViT-B/16 checkpoint (the reference downloads both);
    ``--random_init`` builds SD-1.x- / ViT-B/16-shaped synthetic weights (``--tiny``: small test sizes).
  * under ``torch.distributed.run`` the dataset entries are sharded across the ranks, one process per
    GPU, no data-path collective (BASELINE configs[4]).
The ``ef_p2p`` comparison baseline of the reference driver (Edit Friendly, main_edit.py:218-223, inversion/ef.py) runs through
``edit_ef.py``, which calls ``main`` here with ``modes=("ef_p2p",)``: like the text drivers (main_baselines.py), the h-Edit
driver itself refuses the comparison modes.  ``ef_p2p`` differentiates the style loss through the eps-network, so it builds the
UNet with its input-gradient pass (``args.unet_grad``), passes ``cfg_scales = [cfg_src, cfg_tar]`` and takes its weight from
``--weight_edit_clip_for_ef``.  The output folder keeps the reference's string, which prints ``w_style_{args.weight_edit_clip}``
(main_edit.py:97) even in that mode: the folder of an ``ef_p2p`` run names the h-Edit weight, not the one it used.
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.clip_guidance import CLIPEncoder  # noqa: E402
from hedit.inversion.ef_style import ef_p2p  # noqa: E402
from hedit.inversion.h_edit import h_Edit_p2p_implicit  # noqa: E402
from hedit.p2p.ptp_classes import ControllerBatch  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402
from hedit.utils import dataset_from_json  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument('--dataset', type=str, default="./assets/demo/")
    p.add_argument('--output_path', type=str, default="./results/demo/")
    p.add_argument("--mode", default="h_edit_R_p2p", help="modes: h_edit_R_p2p (ef_p2p: edit_ef.py)")
    p.add_argument("--num_diffusion_steps", type=int, default=50)
    p.add_argument("--skip", type=int, default=0)
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--cfg_src", type=float, default=1.0)
    p.add_argument("--cfg_src_edit", type=float, default=5.0)
    p.add_argument("--cfg_tar", type=float, default=7.5)
    p.add_argument("--implicit", action='store_false', help="Use implicit form of h-Edit")
    p.add_argument("--optimization_steps", type=int, default=1)
    DR.add_family_flags(p, "p2p")
    p.add_argument("--weight_edit_clip", type=float, default=0.5)
    p.add_argument("--weight_edit_clip_for_ef", type=float, default=1.5)
    DR.add_build_flags(p)
    p.add_argument("--clip_path", type=str, default=None, help="local OpenAI CLIP ViT-B/16 checkpoint (.pt)")
    return p


def load_style_encoder(args, ref_path, device):
    if args.clip_path:
        return CLIPEncoder(need_ref=True, ref_path=ref_path, clip_path=args.clip_path, device=device)
    if not args.random_init:
        raise SystemExit("give --clip_path FILE (local OpenAI CLIP ViT-B/16 checkpoint) or --random_init")
    if args.tiny:
        from hedit.clip_guidance.base_clip import ClipVisualPrefix
        m = ClipVisualPrefix(width=64, layers=3, heads=1, patch_size=32, input_resolution=224).init_random(args.seed)
        return CLIPEncoder(need_ref=True, ref_path=ref_path, clip_model=m.half(), device=device)
    return CLIPEncoder(need_ref=True, ref_path=ref_path, device=device, seed=args.seed)


def edit_group(args, model, entries, scale, size, device):
    """The n entries [(key, item, image_path, save_path)] of one group.  One entry goes through the reference-signature
    functions (main_edit.py:103-247), several in lock-step through the batched engine, where every image keeps its own
    style reference (CLIPEncoder.get_gram_matrix_residual reads batch item 0 only, clip_guidance/base_clip.py:60-65) on ONE
    copy of the encoder (CLIPEncoder.sibling)."""
    encs = []
    for _, item, _, _ in entries:
        encs.append(encs[0].sibling(args.dataset + item['style']) if encs else load_style_encoder(args, args.dataset + item['style'], device))
    DR.set_scheduler(model, args.num_diffusion_steps, False)
    after_skip_steps = args.num_diffusion_steps - args.skip
    pairs = [[DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])] for _, item, _, _ in entries]
    cfg_scales = [args.cfg_src, args.cfg_src_edit, args.cfg_tar]
    w0 = DR.encode_images(model, entries, scale, size, device, "p2p")
    engine = DR.lock_step_engine(model, len(entries))
    if args.mode == "ef_p2p" and engine:
        # image by image, so that the forward process draws the numbers of the one-at-a-time run: the group's results are
        # then those runs' bit for bit (the inversion is T two-row passes, a small part of this mode's step)
        inv = [DR.invert(args, model, w0[i:i + 1], p[0]) for i, p in enumerate(pairs)]
        zs, wts, eta = torch.stack([v[0] for v in inv], 1), torch.stack([v[1] for v in inv], 1), inv[0][2]
    else:
        zs, wts, eta = DR.invert(args, model, w0, [p[0] for p in pairs] if engine else pairs[0][0], engine)
    # main_edit.py:185-214: no local blend, no heuristic equaliser for the combined task; the dataset's blended word is
    # re-weighted by 2.0; Replace whenever source and target have the same number of words
    ctrls = [DR.p2p_controller(args, model, item, after_skip_steps, replace=len(p[0].split(" ")) == len(p[1].split(" ")),
                               local_blend=False) for (_, item, _, _), p in zip(entries, pairs)]
    controller = ControllerBatch(ctrls) if engine else ctrls[0]
    register_attention_control(model, controller)
    if args.mode == "ef_p2p":                            # main_edit.py:218-223; a group in lock-step, one encoder per image
        edited, _ = ef_p2p(model, encs if engine else encs[0], xT=wts[after_skip_steps].contiguous(), etas=eta,
                           prompts=pairs if engine else pairs[0], cfg_scales=[args.cfg_src, args.cfg_tar], prog_bar=True,
                           zs=zs[:after_skip_steps], controller=controller, weight_edit_clip=args.weight_edit_clip_for_ef,
                           is_ddim_inversion=False, per_image=True)
        model.unet.zero_grad()
    elif engine:
        edited, _ = engine.run(wts[after_skip_steps].contiguous(), zs[:after_skip_steps].contiguous(), pairs, cfg_scales, controller,
                               eta=eta, p2p=True, implicit=True, K=args.optimization_steps, after_skip_steps=after_skip_steps,
                               ddim_inv=False, fuse_src_pass=True, style=(encs, args.weight_edit_clip))
    else:
        edited, _ = h_Edit_p2p_implicit(model, image_encoder=encs[0], xT=wts[after_skip_steps], eta=eta, prompts=pairs[0],
                                        cfg_scales=cfg_scales, prog_bar=True, zs=zs[:after_skip_steps], controller=controller,
                                        weight_edit_clip=args.weight_edit_clip, optimization_steps=args.optimization_steps,
                                        after_skip_steps=after_skip_steps, is_ddim_inversion=False)
    with torch.no_grad():
        x0_dec = model.vae.decode(1 / scale * edited).sample
        for i, enc in enumerate(encs):
            print(f'loss from CLIP: {torch.linalg.norm(enc.get_gram_matrix_residual(x0_dec[i:i + 1])).item()}')
    return DR.save_group(x0_dec, entries)


def main(argv=None, modes=("h_edit_R_p2p",)):
    """modes: what this entry runs -- ("h_edit_R_p2p",) for this driver, ("ef_p2p",) from edit_ef.py"""
    args = build_parser().parse_args(argv)
    assert args.eta == 1.0, "eta should be set to 1.0 for this experiment"
    assert args.optimization_steps == 1, "we have not tested multiple optimization steps for this experiment"
    assert args.implicit, "we only demo the implicit form for this experiment"
    if args.mode not in modes or args.mode not in ("h_edit_R_p2p", "ef_p2p"):
        raise NotImplementedError(f"mode {args.mode}: this driver runs {', '.join(modes)} (ef_p2p: edit_ef.py)")
    if args.mode == "ef_p2p":
        args.unet_grad = True                   # Edit Friendly differentiates through the eps-network
    print(f'Arguments: {args}')
    run = DR.start_run(args, lambda: dataset_from_json(args.dataset + "demo.json"),
                       no_vae="the checkpoint has no vae/ sub-folder: the style closure decodes through it")
    todo = [(key, item, args.dataset + item['image_path']) for key, item in run.full_data.items()]
    sub = DR.out_subdir(args, run.time_stamp, DR.family_tail(args, "p2p"), weight=("w_style", args.weight_edit_clip))
    return DR.run_groups(args, run, todo, args.dataset, sub, edit_group)


if __name__ == "__main__":
    main()
