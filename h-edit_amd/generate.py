#!/usr/bin/env python3
"""Prompt-to-Prompt generation driver on the HIP path: a source / target image pair from ONE noise sample under a
Prompt-to-Prompt controller (the original workflow of the reference's ``text-guided/p2p/ptp_utils.py``:
text2image_ldm_stable :231-275), and the cross-attention maps that decide LocalBlend's mask.  No image is inverted, so it
is the quickest way to check a controller's settings before a long real-image run.

  --prompts FILE   yaml or json list of {source, target, blend_word?, is_replace?, seed?, guidance_scale?}
                   (blend_word: "src_word tar_word" or a list of two; is_replace: the Replace controller instead of Refine)
  --model_path DIR | --random_init [--tiny], --native_text, --batch N, --seed: as in the editing drivers
  --show_attention RES [--from_where up down]: also the target prompt's aggregated RES x RES cross maps, one tile per token

Per entry NNN it writes NNN_source.png, NNN_target.png and, with --show_attention, NNN_cross_attention.png into
--output_path.  ``--batch N`` generates N entries in lock-step (hedit.p2p.ptp_utils.text2image_batch over a
ControllerBatch); the kernels are batch-invariant, so the files are byte-identical to ``--batch 1``.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

from hedit import driver as DR  # noqa: E402
from hedit.p2p import ptp_utils  # noqa: E402
from hedit.p2p.ptp_classes import ControllerBatch, show_cross_attention  # noqa: E402
from hedit.p2p.ptp_controller_utils import make_controller  # noqa: E402

_ROOT = "<entries>/"        # run_groups names an output after its input: entry NNN "is read" from <entries>/NNN


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument("--prompts", type=str, default=None, help="yaml or json list of {source, target, blend_word?, is_replace?, "
                                                             "seed?, guidance_scale?}")
    p.add_argument("--output_path", type=str, default="./results/generate")
    p.add_argument("--num_inference_steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--cross_replace_steps", type=float, default=0.8)
    p.add_argument("--self_replace_steps", type=float, default=0.4)
    p.add_argument("--show_attention", type=int, default=None, metavar="RES")
    p.add_argument("--from_where", nargs="+", default=["up", "down"], choices=["down", "mid", "up"])
    DR.add_build_flags(p)
    return p


def read_prompts(path):
    """the entries of a prompt file, each also under the keys the stand-in tokenizer's prescan reads"""
    with open(path) as f:
        if path.endswith((".yaml", ".yml")):
            try:
                import yaml
            except ImportError:
                raise SystemExit("--prompts: a yaml file needs PyYAML; give a json file instead")
            data = yaml.safe_load(f)
        else:
            data = json.load(f)
    if not isinstance(data, list) or not data:
        raise SystemExit(f"{path}: a non-empty list of entries expected")
    known = {"source", "target", "blend_word", "is_replace", "seed", "guidance_scale"}
    out = []
    for i, item in enumerate(data):
        if not isinstance(item, dict) or not {"source", "target"} <= set(item) or set(item) - known:
            raise SystemExit(f"{path}: entry {i} must have source and target and may have {sorted(known - {'source', 'target'})}")
        out.append(dict(item, source_prompt=item["source"], target_prompt=item["target"]))
    return out


def entry_controller(args, model, item):
    bw = item.get("blend_word")
    if isinstance(bw, str):
        bw = bw.split(" ")
    if bw is not None and len(bw) != 2:
        raise SystemExit(f"blend_word {item['blend_word']!r}: one source word and one target word expected")
    return make_controller(prompts=[item["source"], item["target"]], is_replace_controller=bool(item.get("is_replace", False)),
                           cross_replace_steps=args.cross_replace_steps, self_replace_steps=args.self_replace_steps,
                           blend_word=((bw[0],), (bw[1],)) if bw else None, equilizer_params=None,
                           num_steps=args.num_inference_steps, tokenizer=model.tokenizer, device=model.device)


def generate_group(args, model, entries, scale, size, device):
    """The n entries [(key, item, _, stem)] of one group: one controller per entry, x_T from the entry's seed on the CPU,
    the lock-step generation loop, VAE decode, PNGs -> the written paths."""
    from PIL import Image
    n = len(entries)
    items = [e[1] for e in entries]
    pairs = [[it["source"], it["target"]] for it in items]
    ctrls = [entry_controller(args, model, it) for it in items]
    controller = ControllerBatch(ctrls) if n > 1 else ctrls[0]
    gens = [torch.Generator().manual_seed(int(it.get("seed", args.seed))) for it in items]
    guidance = [float(it.get("guidance_scale", args.guidance_scale)) for it in items] * 2        # rows [src]*n, [tar]*n
    latents, _ = ptp_utils.text2image_batch(model, pairs, controller, args.num_inference_steps, guidance, generators=gens)
    images = ptp_utils.latent2image(model.vae, latents)
    written = []
    for i, entry in enumerate(entries):
        stem = entry[3]
        os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
        for img, tag in ((images[i], "source"), (images[n + i], "target")):
            Image.fromarray(img).save(f"{stem}_{tag}.png")
            written.append(f"{stem}_{tag}.png")
        if args.show_attention is not None:
            grid = show_cross_attention(controller, args.show_attention, args.from_where, select=1, prompts=pairs[i],
                                        tokenizer=model.tokenizer, image=i if n > 1 else None)
            grid.save(f"{stem}_cross_attention.png")
            written.append(f"{stem}_cross_attention.png")
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.prompts:
        raise SystemExit("give --prompts FILE (yaml or json list of {source, target, ...})")
    run =DR.start_run(args, lambda: read_prompts(args.prompts),
                       no_vae="the checkpoint has no vae/ sub-folder: the generated latents cannot be decoded")
    todo = [(f"{i:03d}", item, f"{_ROOT}{i:03d}") for i, item in enumerate(run.full_data)]
    return DR.run_groups(args, run, todo, _ROOT, "", generate_group)


if __name__ == "__main__":
    main()
