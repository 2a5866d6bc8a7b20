#!/usr/bin/env python3
"""Demo driver on the HIP path: same flags, dataset format (``<data_path>/demo.yaml``: a list of
``image / source_prompt / target_prompt / blended_word / editing_instruction`` entries) and output-path
scheme as the reference's ``text-guided/main_demo.py`` (:49-84 flags, :113-118 strings, :124-262 loop)
for the h-Edit modes (h_edit_R, h_edit_R_p2p, h_edit_D_p2p; explicit or ``--implicit``).  It is main_p2p.py
over another dataset file, with one rule of its own: it picks the Replace controller whenever source and target
have the same number of words (:181) and merges the heuristic equaliser of ``preprocessing`` with the dataset's
blended word (:196-213).

Differences, all additive:
  * ``--model_path DIR``: a LOCAL checkpoint directory in the diffusers layout (no network here);
    ``--random_init`` builds SD-1.x-shaped synthetic weights instead (``--tiny`` = the small test
    configuration at 256x256).
  * launched under ``torch.distributed.run`` the dataset entries are sharded across the ranks
    (one process per GPU, no data-path collective).
The comparison baselines of the reference driver (ef, ef_p2p, nmg_p2p, pnp_inv_p2p) are not part of
this build and are refused.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import main_p2p  # noqa: E402
from hedit import driver as DR  # noqa: E402
from hedit.p2p.ptp_controller_utils import preprocessing  # noqa: E402


def build_parser():
    return main_p2p.build_parser("./results/demo", data_path="./assets/demo", categories=False)


def read_demo_file(data_path):
    import yaml
    with open(data_path + "/demo.yaml") as f:
        return yaml.safe_load(f)


def replace_rule(args, key, item):
    src, tar = DR.clean(item["original_prompt"]), DR.clean(item["editing_prompt"])
    return dict(replace=len(src.split(" ")) == len(tar.split(" ")), eq_extra=preprocessing(src, tar, is_global_edit=True)[1])


def main(argv=None):
    args = build_parser().parse_args(argv)
    main_p2p.check_mode(args)
    run = DR.start_run(args, lambda: read_demo_file(args.data_path))
    todo = [(str(idx), {"original_prompt": it.get("source_prompt", ""), "editing_prompt": it.get("target_prompt", ""),
                        "blended_word": it["blended_word"]}, args.data_path + it["image"])
            for idx, it in enumerate(run.full_data)]
    tail = DR.family_tail(args, "p2p") if args.mode in ('h_edit_D_p2p', 'h_edit_R_p2p') else '_'
    return DR.run_groups(args, run, todo, args.data_path, DR.out_subdir(args, run.time_stamp, tail), main_p2p.edit_group,
                         rule=replace_rule)


if __name__ == "__main__":
    main()
