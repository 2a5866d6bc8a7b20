#!/usr/bin/env python3
"""The combined text + style task's comparison column on the HIP path: Edit Friendly with P2P (``--mode ef_p2p`` of the
reference's text-guided-n-style/main_edit.py:46,218-223; inversion/ef.py).  Same flags, dataset format and output folder scheme
as main_edit.py, whose machinery it runs with the ``ef_p2p`` mode enabled: SD UNet with its input-gradient pass
(``UNet2DConditionModel(grad=True)``), edit-friendly DDPM inversion, ``hedit.inversion.ef_style.ef_p2p`` with the reference's
arguments (``cfg_scales = [cfg_src, cfg_tar]``, ``weight_edit_clip = --weight_edit_clip_for_ef``, the controller rule of the
h-Edit mode: equalizer 2.0, no local blend, Replace on equal word counts); ``--batch`` is lock-step with ``per_image=True``.  A
driver of its own because the h-Edit driver refuses the comparison modes, as main_baselines.py is for the text drivers.  It is
not named main_*.py: those are the drivers with a parser of their own, each pinned in tests/golden/g25_driver_cli.json, and this
one parses with main_edit.py's.

The output folder keeps the reference's string (main_edit.py:97), which prints ``w_style_{args.weight_edit_clip}`` -- the h-Edit
weight, default 0.5 -- even in this mode; the weight the run uses, ``--weight_edit_clip_for_ef``, is not in the name."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import main_edit  # noqa: E402


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--mode" not in argv:
        argv += ["--mode", "ef_p2p"]
    return main_edit.main(argv, modes=("ef_p2p",))


if __name__ == "__main__":
    main()
