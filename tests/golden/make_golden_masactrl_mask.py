#!/usr/bin/env python3
"""Writes g28_masactrl_mask.npz: the outputs of the reference's ``MutualSelfAttentionControlMask`` and
``MutualSelfAttentionControlMaskAuto`` (text-guided/masactrl/masactrl.py:71-286), UNMODIFIED, on the seeded inputs of
tests/helpers/masactrl_mask_ref.py -- n = 1 (the reference's 4 rows), 2 heads, N = 64 and 256; given masks (a mixed pair and
an empty-class pair) and auto masks over seeded fake cross maps; the two target rows of every output are kept.  Needs the reference tree (imported as make_golden.py imports
it; torchvision, which is not installed, is stubbed: save_image is never reached); the test reads the committed file only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from helpers import masactrl_mask_ref as MR  # noqa: E402
from make_golden import _stub, import_reference  # noqa: E402

HEADS, D = 2, 2
TARGET_ROWS = [1, 3]          # the rows the editors change; the source rows are plain attention
CASES_GIVEN = [("mixed", 64, 101), ("mixed", 256, 102), ("empty", 64, 103), ("empty", 256, 104)]
CASES_AUTO = [(64, 0.1, [1], [1], 201), (256, 0.1, [1, 2], [3], 202), (256, 0.5, [2], [2], 203)]


def flat(t):
    """(4, h, n, d) -> the reference's (batch * heads, n, d), batch-major"""
    return t.reshape(4 * t.shape[1], t.shape[2], t.shape[3])


def main():
    import_reference()
    tv = _stub("torchvision")
    tv.utils = _stub("torchvision.utils", save_image=lambda *a, **k: None)
    import masactrl.masactrl_utils as mu
    pkg = _stub("masa_ctrl")
    pkg.masactrl_utils = mu
    sys.modules["masa_ctrl.masactrl_utils"] = mu
    import masactrl.masactrl as mm
    scale = D ** -0.5
    unused = torch.zeros(4 * HEADS, 1, 1)             # `sim` and `attn` of a self-attention call: sliced, never read
    out = {}
    for kind, N, seed in CASES_GIVEN:
        q, k, v = MR.golden_qkv(seed, HEADS, D, N)
        ms, mt = MR.golden_given_masks(kind, seed)
        ed = mm.MutualSelfAttentionControlMask(0, 0, mask_s=ms, mask_t=mt)
        got = ed.forward(flat(q), flat(k), flat(v), unused, unused, False, "down", HEADS, scale=scale)
        out[f"given_{kind}_{N}"] = got[TARGET_ROWS].numpy()
    for N, thres, ref_idx, cur_idx, seed in CASES_AUTO:
        q, k, v = MR.golden_qkv(seed, HEADS, D, N)
        ed = mm.MutualSelfAttentionControlMaskAuto(0, 0, thres=thres, ref_token_idx=ref_idx, cur_token_idx=cur_idx)
        vc = torch.zeros(4 * HEADS, 77, D)
        for p in MR.golden_cross(seed, HEADS):
            ed.forward(None, None, vc, None, p.reshape(4 * HEADS, 256, 77), True, "down", HEADS, scale=scale)
        got = ed.forward(flat(q), flat(k), flat(v), unused, unused, False, "down", HEADS, scale=scale)
        out[f"auto_{N}_{thres}_{seed}"] = got[TARGET_ROWS].numpy()
    # auto with no map collected: unmasked mutual attention (:247-250)
    q, k, v = MR.golden_qkv(301, HEADS, D, 64)
    ed = mm.MutualSelfAttentionControlMaskAuto(0, 0)
    out["auto_nomap_64"] = ed.forward(flat(q), flat(k), flat(v), unused, unused, False, "down", HEADS, scale=scale)[TARGET_ROWS].numpy()
    np.savez_compressed(os.path.join(HERE, "g28_masactrl_mask.npz"), **out)
    print("wrote", len(out), "arrays", {k: a.shape for k, a in out.items()})


if __name__ == "__main__":
    main()
