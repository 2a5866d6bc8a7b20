"""The PIE-Bench edit mask of a mapping-file entry (text-guided/evaluation/evaluation.py:9-25), shared by the evaluator
(evaluation/evaluation.py) and the MasaCtrl driver's ``--masa_mask pie``.  numpy only."""
import numpy as np


def mask_decode(encoded_mask, image_shape=(512, 512)):
    """PIE-Bench run-length mask: pairs (start, length) over the flattened image; the one-pixel border is forced to 1
    ("to avoid annotation errors in boundary", evaluation.py:9-25)."""
    length = image_shape[0] * image_shape[1]
    flat = np.zeros((length,))
    enc = np.asarray(encoded_mask, dtype=np.int64).reshape(-1, 2) if len(encoded_mask) else np.zeros((0, 2), dtype=np.int64)
    for start, run in enc:
        flat[start:start + max(0, min(run, length - start))] = 1
    m = flat.reshape(image_shape[0], image_shape[1])
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    return m
