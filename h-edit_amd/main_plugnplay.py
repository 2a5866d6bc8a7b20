#!/usr/bin/env python3
"""h-Edit with Plug-and-Play on the HIP path: same flags, dataset format and output-path scheme as the reference's
``text-guided/main_plugnplay.py`` (:56-87 flags, :117-118 strings, :124-248 loop) for the h-Edit modes
(``h_edit_R_pnp``, ``h_edit_D_pnp``).  Additions: ``--model_path`` / ``--random_init`` / ``--tiny`` / ``--seed`` as in
main_p2p.py (``--tiny`` = the four-level toy UNet: the injection indexes up_blocks[1..3]); entries are sharded
over ranks under torch.distributed.run.  The comparison baselines (ef_pnp, pnp_inv_w_pnp, nt_pnp, np_pnp, nmg_pnp)
are not part of this build and are refused."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from hedit import driver as DR  # noqa: E402
from hedit.inversion.pnp_h_edit import h_Edit_PnP_implicit  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    DR.add_reference_flags(p, "./results/pnp", "h_edit_R_pnp", 1.0, "modes: h_edit_R_pnp, h_edit_D_pnp")
    DR.add_family_flags(p, "pnp")
    DR.add_build_flags(p)
    return p


def edit_group(args, model, entries, scale, size, device):
    """The n entries [(key, item, image_path, save_path)] of one group.  One entry goes through the reference-signature
    functions (main_plugnplay.py:124-248), several in lock-step through hedit.engine.HEditEngine.run_pnp (the injected
    pass has rows [x_orig|src]*n, [x_k|tar]*n and row n + i takes row i's q, k / features): the same arithmetic per image."""
    is_ddim_inversion = args.eta == 0
    DR.set_scheduler(model, args.num_diffusion_steps, is_ddim_inversion)
    after = args.num_diffusion_steps - args.skip
    w0 = DR.encode_images(model, entries, scale, size, device, "pnp")
    pairs = [[DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])] for _, item, _, _ in entries]
    cfg_scales = [args.cfg_src, args.cfg_src_edit, args.cfg_tar]
    engine = DR.lock_step_engine(model, len(entries))
    zs, wts, eta = DR.invert(args, model, w0, [p[0] for p in pairs] if engine else pairs[0][0], engine)
    DR.register_pnp(model, after, args.pnp_f_t, args.pnp_attn_t)
    if engine:
        edited, _ = engine.run_pnp(wts[after].contiguous(), zs[:after].contiguous(), pairs, cfg_scales, eta=eta,
                                   K=args.optimization_steps, after_skip_steps=after, ddim_inv=is_ddim_inversion)
    else:
        edited, _ = h_Edit_PnP_implicit(model, xT=wts[after], eta=eta, prompts=pairs[0], cfg_scales=cfg_scales, prog_bar=True,
                                        zs=zs[:after], optimization_steps=args.optimization_steps, after_skip_steps=after,
                                        is_ddim_inversion=is_ddim_inversion)
    return DR.save_group(model.vae.decode(1 / scale * edited).sample, entries)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == "h_edit_D_pnp":
        assert args.eta == 0.0, "eta should be 0.0 for h-Edit-D"
    elif args.mode == "h_edit_R_pnp":
        assert args.eta == 1.0, "eta should be 1.0 for h-Edit-R"
    else:
        raise NotImplementedError(f"mode {args.mode}: only h_edit_R_pnp / h_edit_D_pnp are built")
    print(f'Arguments: {args}')
    return DR.run_pie_bench(args, DR.family_tail(args, "pnp"), edit_group, family="pnp")


if __name__ == "__main__":
    main()
