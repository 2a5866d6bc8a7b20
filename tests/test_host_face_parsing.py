"""CPU (no GPU): the face-parsing parameter container hedit.arcface.FaceParsing against the reference's parameter table
(tests/golden/g17_face_parsing.json, written by RUNNING the reference: tests/golden/make_golden_parsing.py), strict
loading, the configurations and sizes it refuses, and the ABI of the native network in both builds of the library."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.parsing import parsing_state_dict  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.arcface import FaceParsing, face_mask  # noqa: E402

META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_face_parsing.json")))


def test_parameter_table_is_the_reference_one():
    m = FaceParsing()
    table = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert table == META["params"] and len(table) == 136
    assert sum(p.numel() for p in m.parameters()) == META["n_params"] == 1944355
    assert m.param_shapes == {k: tuple(s) for k, s in META["params"] if not k.endswith("num_batches_tracked")}
    assert m.training    # the reference never calls .eval() on it


def test_strict_load():
    m = FaceParsing()
    sd = parsing_state_dict({k: tuple(s) for k, s in META["params"]})
    m.load_state_dict(sd)
    assert torch.equal(m.up_concat4.up.weight, sd["up_concat4.up.weight"])
    # the integer BatchNorm counters are optional (a broadcast checkpoint does not carry them)
    m.load_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "final.bias"})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict(dict(sd, **{"final.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(dict(sd, **{"final.bias": torch.zeros(20)}))


@pytest.mark.parametrize("kw", [dict(feature_scale=2), dict(n_classes=11), dict(is_deconv=False), dict(in_channels=1),
                                dict(is_batchnorm=False)])
def test_unsupported_configurations_are_refused(kw):
    with pytest.raises(NotImplementedError):
        FaceParsing(**kw)


@pytest.mark.parametrize("shape", [(1, 3, 40, 32), (1, 3, 32, 24), (1, 3, 8, 8), (1, 1, 32, 32), (3, 32, 32)])
def test_sizes_that_are_not_multiples_of_16_are_refused(shape):
    with pytest.raises(ValueError):
        FaceParsing()(torch.zeros(shape))


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="HIP executor"):
        FaceParsing()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="HIP executor"):
        face_mask(torch.zeros(1, 1, 32, 32, dtype=torch.int64))
    with pytest.raises(ValueError):
        face_mask(torch.zeros(1, 1, 32, 32, dtype=torch.int64), kernel_size=12)


def test_abi_is_declared_and_exported_by_both_builds():
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    want = {f"hedit_faceparse_{s}" for s in ("create", "destroy", "num_params", "param_name", "param_shape", "load", "missing",
                                             "finalize", "workspace_bytes", "labels")} | {"hedit_face_mask", "hedit_face_mask_workspace_bytes"}
    assert want <= set(re.findall(r"\b(hedit_[a-z0-9_]+)\s*\(", hdr))
    assert want <= set(_lib.EXPORTS)
    for path in (_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), "libhedit_hip_f16.so")):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, n) for n in want), path
    lib = _lib.lib()
    # the mask workspace needs no device: two fields, the per-image maxima and the cone table
    assert lib.hedit_face_mask_workspace_bytes(2, 64, 48) >= 2 * 2 * 64 * 48 * 4
    assert lib.hedit_face_mask_workspace_bytes(0, 64, 48) == 0
