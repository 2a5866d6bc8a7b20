#!/usr/bin/env python3
"""Writes g26_aggregate_attention.npz: the reference's ``aggregate_attention`` (text-guided/p2p/ptp_classes.py:298-309) over
its own ``AttentionStore`` filled with the seeded fake steps of tests/helpers/p2p_generate_ref.py.  Needs the reference tree
(imported as make_golden.py imports it: cv2, diffusers and nltk stubbed); the test reads the committed file only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from helpers import p2p_generate_ref as PR  # noqa: E402
from make_golden import import_reference  # noqa: E402

SEED = 26
CASES = [(8, ("up", "down"), True), (8, ("down",), True), (4, ("down", "mid", "up"), True), (4, ("mid",), True),
         (8, ("up", "down"), False), (4, ("up",), False)]


def main():
    ref = import_reference()
    store = PR.fill_store(ref.pc.AttentionStore(), PR.fake_steps(SEED))
    out = {}
    for res, where, is_cross in CASES:
        for select in (0, 1):
            got = ref.pc.aggregate_attention(store, res, list(where), is_cross, select, prompts=["a", "b"])
            out[f"res{res}_{'-'.join(where)}_{'cross' if is_cross else 'self'}_{select}"] = got.numpy()
    np.savez_compressed(os.path.join(HERE, "g26_aggregate_attention.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
