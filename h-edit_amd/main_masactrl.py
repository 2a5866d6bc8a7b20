#!/usr/bin/env python3
"""h-Edit with MasaCtrl on the HIP path: same flags, dataset format and output-path scheme as the reference's
``text-guided/main_masactrl.py`` (:55-88 flags, :118-124 strings, :128-241 loop) for the h-Edit modes
(``h_edit_D_masactrl``, ``h_edit_R_masactrl``).  Like the reference the source prompt is the empty string
(:178).  (The reference reads ``args.LAYER`` for the ``--layer`` flag, :198, which argparse never sets; this
driver uses ``args.layer``.)  Additions: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed`` as in
main_p2p.py; entries are sharded over ranks under torch.distributed.run.  The comparison baselines
(pnp_inv_masactrl, ef_masactrl) are not part of this build and are refused.

``--masa_mask {none,pie}`` (an addition, default ``none``: flags, outputs and directory names exactly as without it):
``pie`` runs the mask-guided editor ``MutualSelfAttentionControlMask`` (masactrl/masactrl.py:71-148) with ``mask_s = mask_t =``
the entry's PIE-Bench edit mask and appends ``_mask_pie`` to the output directory's name.  There is no flag for the auto
variant (``MutualSelfAttentionControlMaskAuto``): it takes its source mask from the cross-attention map of a source-prompt
token, and this driver, like the reference's, runs with an empty source prompt."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.inversion.masactrl_h_edit import h_Edit_masactrl_implicit  # noqa: E402
from hedit.masactrl import (MutualSelfAttentionControl, MutualSelfAttentionControlMask,  # noqa: E402
                            regiter_attention_editor_diffusers)
from hedit.pie_mask import mask_decode  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    DR.add_reference_flags(p, "./results/masactrl", "h_edit_D_masactrl", 0.0, "modes: h_edit_D_masactrl, h_edit_R_masactrl")
    DR.add_family_flags(p, "masactrl")
    DR.add_build_flags(p)
    # (opt-in like --native_text: absent from the namespace unless given, so the default namespace stays the reference's)
    p.add_argument("--masa_mask", choices=("none", "pie"), default=argparse.SUPPRESS,
                   help="none (default) | pie: mask-guided MasaCtrl with the entry's PIE-Bench edit mask as source and target mask")
    return p


def masa_mask(args):
    return getattr(args, "masa_mask", "none")


def output_tail(args):
    """the end of the output sub-directory's name: the family's, plus _mask_pie under --masa_mask pie"""
    return DR.family_tail(args, "masactrl") + ("_mask_pie" if masa_mask(args) == "pie" else "")


def make_editor(args, entries):
    if masa_mask(args) == "none":
        return MutualSelfAttentionControl(args.step, args.layer)
    import numpy as np
    import torch
    masks = torch.from_numpy(np.stack([mask_decode(item.get("mask", [])) for _, item, _, _ in entries])).float()   # (n, 512, 512)
    return MutualSelfAttentionControlMask(args.step, args.layer, mask_s=masks, mask_t=masks)


def edit_group(args, model, entries, scale, size, device):
    """The n entries [(key, item, image_path, save_path)] of one group.  One entry goes through the reference-signature
    functions (main_masactrl.py:128-241), several in lock-step through hedit.engine.HEditEngine (rows [x_orig|null]*n,
    [x_k|null]*n, [x_orig|src]*n, [x_k|tar]*n: the mutual self-attention plan already maps row (kind, i) to the source
    row of image i): the same arithmetic per image."""
    n = len(entries)
    is_ddim_inversion = args.eta == 0
    DR.set_scheduler(model, args.num_diffusion_steps, is_ddim_inversion)
    after = args.num_diffusion_steps - args.skip
    w0 = DR.encode_images(model, entries, scale, size, device, "masactrl")
    src_p = [""] * n                      # MasaCtrl runs without the source prompt (main_masactrl.py:178)
    tar_p = [DR.clean(item["editing_prompt"]) for _, item, _, _ in entries]
    cfg_scales = [args.cfg_src, args.cfg_src_edit, args.cfg_tar]
    engine = DR.lock_step_engine(model, n)
    zs, wts, eta = DR.invert(args, model, w0, src_p if engine else src_p[0], engine)
    editor = make_editor(args, entries)
    regiter_attention_editor_diffusers(model, editor)
    if engine:
        edited, _ = engine.run(wts[after].contiguous(), zs[:after].contiguous(), [[a, b] for a, b in zip(src_p, tar_p)], cfg_scales,
                               editor, eta=eta, p2p=True, implicit=True, K=args.optimization_steps, after_skip_steps=after,
                               ddim_inv=is_ddim_inversion, rec_pull=False)
    else:
        edited, _ = h_Edit_masactrl_implicit(model, xT=wts[after], eta=eta, prompts=[src_p[0], tar_p[0]], cfg_scales=cfg_scales,
                                             prog_bar=True, zs=zs[:after], optimization_steps=args.optimization_steps,
                                             after_skip_steps=after, is_ddim_inversion=is_ddim_inversion)
    return DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == "h_edit_D_masactrl":
        assert args.eta == 0.0, "eta should be 0.0 for h-Edit-D"
    elif args.mode == "h_edit_R_masactrl":
        assert args.eta == 1.0, "eta should be 1.0 for h-Edit-R"
    else:
        raise NotImplementedError(f"mode {args.mode}: only h_edit_D_masactrl / h_edit_R_masactrl are built")
    print(f'Arguments: {args}')
    return DR.run_pie_bench(args, output_tail(args), edit_group)


if __name__ == "__main__":
    main()
