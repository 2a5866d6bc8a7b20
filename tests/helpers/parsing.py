"""Hash-seeded weights of the face-parsing network (tests/golden/make_golden_parsing.py and the tests regenerate them from
the parameter names alone; the fixture stores no weights)."""
import zlib

import numpy as np
import torch

from .tiny import hash_normal


def parsing_state_dict(shapes):
    """{name: tensor} for the reference's FaceParsing() state_dict {name: shape}.  The running statistics are far from
    what the layers see (so eval mode and batch statistics give clearly different labels)."""
    sd = {}
    for name, shape in shapes.items():
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros(shape, dtype=torch.long)
            continue
        v = hash_normal(tuple(shape) if len(shape) else (1,), zlib.crc32(name.encode()) % 100003).reshape(shape)
        if name.endswith("running_var"):
            v = 0.5 + v.abs()
        elif name.endswith("running_mean"):
            v = 0.3 * v
        elif len(shape) > 1:
            v = v * float(np.prod(shape[1:])) ** -0.5
        elif name.endswith("weight"):
            v = 1.0 + 0.1 * v
        else:
            v = 0.05 * v
        sd[name] = v
    return sd
