#!/usr/bin/env python3
"""The face task's comparison column on the HIP path: Edit Friendly (``--mode ef`` of the reference's
face-swapping/main_edit.py:46,201-204; inversion/ef.py).  Same flags, dataset format and output folder scheme as
main_edit_face.py (``<output_path>ef/steps_..._skip_..._weight_..._opts_.../item_<ref>_<source>.png``), whose machinery it
runs with the ``ef`` mode enabled: pixel DDPM UNet with its input-gradient pass (``hedit.diffusion.Model(grad=True)``), SDE
inversion, ``hedit.inversion.ef_face.ef`` with the reference's arguments (``soft_face_mask=None``); ``--batch`` is lock-step
with ``per_image=True``.  A driver of its own because the h-Edit driver refuses the comparison modes, as main_baselines.py is
for the text drivers.  ``--weight_edit_face`` keeps the shared parser's default (50); the reference's ``ef`` default is 100."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import main_edit_face  # noqa: E402


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--mode" not in argv:
        argv += ["--mode", "ef"]
    return main_edit_face.main(argv, modes=("ef",))


if __name__ == "__main__":
    main()
