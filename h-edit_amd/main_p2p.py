#!/usr/bin/env python3
"""Text-guided editing driver on the HIP path: same flags, dataset format and output-path scheme as
the reference's ``text-guided/main_p2p.py`` (:38-70 flags, :76-103 strings, :110-275 loop) for the
h-Edit modes (h_edit_R, h_edit_R_p2p, h_edit_D_p2p; explicit or ``--implicit``).

Differences, all additive:
  * ``--model_path DIR``: a LOCAL checkpoint directory in the diffusers layout (no network here);
    ``--random_init`` builds SD-1.x-shaped synthetic weights instead (``--tiny`` = the small test
    configuration at 256x256).
  * launched under ``torch.distributed.run`` the dataset entries are sharded across the ranks
    (one process per GPU, no data-path collective).
  * ``--batch N``: N dataset entries are edited in lock-step by the batched engine (the reference edits one image
    at a time, main_p2p.py:110; images are independent, and the kernels are batch-invariant bit for bit, so every
    image comes out exactly as it does alone -- at several times the throughput).
The comparison baselines of the reference driver (ef, ef_p2p, nmg_p2p, pnp_inv_p2p) are not part of
this build and are refused.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.inversion.p2p_h_edit import (h_Edit_p2p_explicit, h_Edit_p2p_implicit, h_Edit_R_explicit,  # noqa: E402
                                        h_Edit_R_implicit)
from hedit.p2p.ptp_classes import AttentionStore, ControllerBatch  # noqa: E402
from hedit.p2p.ptp_utils import register_attention_control  # noqa: E402

# entries for which the reference switches to the Replace controller when source and target have
# the same number of words (main_p2p.py:183-186)
_REPLACE_KEYS_DDIM = {'111000000001', '111000000004', '111000000009', '121000000007', '122000000006',
                      '121000000000', '121000000001'}
_REPLACE_KEYS_DDPM = {'122000000005', '122000000006', '000000000099', '214000000009'}


def build_parser(output_path="./results/p2p", **reference):
    p = argparse.ArgumentParser()
    DR.add_reference_flags(p, output_path, "h_edit_R_p2p", 1.0, "modes: h_edit_R, h_edit_D_p2p, h_edit_R_p2p", **reference)
    DR.add_family_flags(p, "p2p")
    DR.add_build_flags(p)
    return p


def check_mode(args):
    if args.mode == "h_edit_D_p2p":
        assert args.eta == 0.0, "eta should be 0.0 for h-Edit-D"
    elif args.mode in ("h_edit_R", "h_edit_R_p2p"):
        assert args.eta == 1.0, "eta should be 1.0 for h-Edit-R"
    else:
        raise NotImplementedError(f"mode {args.mode}: only the h-Edit modes are built (h_edit_R, h_edit_R_p2p, h_edit_D_p2p)")
    print(f'Arguments: {args}')


def replace_rule(args, key, item):
    """what DR.p2p_controller takes beyond the dataset entry: the Replace controller for the reference's list of entries"""
    same_len = len(DR.clean(item["original_prompt"]).split(" ")) == len(DR.clean(item["editing_prompt"]).split(" "))
    return dict(replace=same_len and key in (_REPLACE_KEYS_DDIM if args.eta == 0 else _REPLACE_KEYS_DDPM))


def edit_group(args, model, entries, scale, size, device, rule=replace_rule):
    """The n entries [(key, item, image_path, save_path)] of one group: VAE encode, inversion, the loop, VAE decode.  One
    entry goes through the reference-signature functions (main_p2p.py:110-275), several in lock-step through
    hedit.engine.HEditEngine (2n-row inversion calls, 4n / 5n-row loop calls, one controller per image in a
    ControllerBatch): the same arithmetic per image.  rule(args, key, item): the driver's choice of controller."""
    n = len(entries)
    is_ddim_inversion = args.eta == 0
    DR.set_scheduler(model, args.num_diffusion_steps, is_ddim_inversion)
    after_skip_steps = args.num_diffusion_steps - args.skip
    pairs = [[DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])] for _, item, _, _ in entries]
    cfg_scales = [args.cfg_src, args.cfg_src_edit, args.cfg_tar]
    w0 = DR.encode_images(model, entries, scale, size, device, "p2p")
    engine = DR.lock_step_engine(model, n)
    zs, wts, eta = DR.invert(args, model, w0, [p[0] for p in pairs] if engine else pairs[0][0], engine)

    p2p = args.mode.endswith('p2p')
    controller = AttentionStore()
    if p2p:
        ctrls = [DR.p2p_controller(args, model, item, after_skip_steps, eq_value=1.25 if args.optimization_steps > 1 else 2.0,
                                   **rule(args, key, item)) for key, item, _, _ in entries]
        controller = ControllerBatch(ctrls) if engine else ctrls[0]
    register_attention_control(model, controller)

    if engine:
        edited, _ = engine.run(wts[after_skip_steps].contiguous(), zs[:after_skip_steps].contiguous(), pairs, cfg_scales, controller,
                               eta=eta, p2p=p2p, implicit=args.implicit, K=args.optimization_steps, w_rec=args.weight_reconstruction,
                               after_skip_steps=after_skip_steps, ddim_inv=is_ddim_inversion, fuse_src_pass=p2p and args.implicit)
    else:
        kw = dict(xT=wts[after_skip_steps], eta=eta, prompts=pairs[0], cfg_scales=cfg_scales, prog_bar=True,
                  zs=zs[:after_skip_steps], controller=controller, after_skip_steps=after_skip_steps,
                  is_ddim_inversion=is_ddim_inversion)
        if args.implicit:
            fn = h_Edit_R_implicit if args.mode == 'h_edit_R' else h_Edit_p2p_implicit
            edited, _ = fn(model, weight_reconstruction=args.weight_reconstruction, optimization_steps=args.optimization_steps, **kw)
        else:
            fn = h_Edit_R_explicit if args.mode == 'h_edit_R' else h_Edit_p2p_explicit
            edited, _ = fn(model, **kw)
    out = DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)
    model.unet.zero_grad()
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_mode(args)
    return DR.run_pie_bench(args, DR.family_tail(args, "p2p") if args.mode in ('h_edit_D_p2p', 'h_edit_R_p2p') else '_', edit_group)


if __name__ == "__main__":
    main()
