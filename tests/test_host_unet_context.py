"""Host: the bound text context of the UNet (hedit_unet_context).  Its four entries are declared in include/hedit.h, exported by
both builds of the library and carry argtypes in hedit/_lib.py; the Python owner (hedit.unet.UNetContext) follows the handle
lifecycle of hedit/native.py -- driven here with CPU tensors against a recording fake of the library, no GPU."""
import contextlib
import ctypes
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib, native  # noqa: E402
from hedit.unet import UNetContext  # noqa: E402

ENTRIES = ["hedit_unet_context_create", "hedit_unet_context_destroy", "hedit_unet_forward_bound", "hedit_unet_forward_shared_bound"]


def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hedit.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert "typedef struct hedit_unet_context hedit_unet_context;" in header
    assert "SNAPSHOT" in header
    res, args = _lib._SIGS["hedit_unet_context_create"]
    assert res is ctypes.c_int and len(args) == 5
    assert _lib._SIGS["hedit_unet_context_destroy"] == (None, [ctypes.c_void_p])
    # the bound forwards take what the plain ones take, the context handle in place of the tensor
    assert _lib._SIGS["hedit_unet_forward_bound"] == _lib._SIGS["hedit_unet_forward"]
    assert _lib._SIGS["hedit_unet_forward_shared_bound"] == _lib._SIGS["hedit_unet_forward_shared"]


@pytest.mark.parametrize("so", ["libhedit_hip.so", "libhedit_hip_f16.so"])
def test_both_libraries_export_the_entries(so):
    path = os.path.join(ROOT, "h-edit_amd", "hedit", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} is not built")
    lib = ctypes.CDLL(path)
    for name in ENTRIES:
        assert hasattr(lib, name), name


class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.log = rc, []

    def hedit_last_error(self):
        return b"fake failure"

    def hedit_unet_context_create(self, h, ctx, rows, stream, out):
        self.log.append(("create", h, rows))
        if self.rc == 0:
            out._obj.value = 0xC0
        return self.rc

    def hedit_unet_context_destroy(self, h):
        self.log.append(("destroy", h.value))


@pytest.fixture
def seams(monkeypatch):
    monkeypatch.setattr(native, "_device_ctx", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(native, "_sync_stream", lambda: None)
    monkeypatch.setattr(_lib, "cur_stream", lambda: None)

    def install(fake):
        monkeypatch.setattr(_lib, "_lib", fake)
        return types.SimpleNamespace(_lib=fake, _h="model", device=torch.device("cpu"), config={"cross_attention_dim": 8})
    return install


def test_owner_lifecycle(seams):
    fake = FakeLib()
    model = seams(fake)
    cx = UNetContext(model, torch.zeros(3, 77, 8))
    assert cx.rows == 3 and cx._h.value == 0xC0 and cx._lib is fake
    assert fake.log == [("create", "model", 3)]
    cx.close()
    cx.close()
    assert cx._h is None and fake.log[1:] == [("destroy", 0xC0)]
    cx2 = UNetContext(model, torch.zeros(1, 77, 8))
    del cx2                                    # dropping the object releases it
    assert fake.log[-1] == ("destroy", 0xC0)


def test_failed_create_leaves_nothing_to_destroy(seams):
    fake = FakeLib(rc=-1)
    model = seams(fake)
    with pytest.raises(_lib.HipError):
        UNetContext(model, torch.zeros(2, 77, 8))
    assert [e[0] for e in fake.log] == ["create"]


def test_rows_are_checked_before_the_library_is_called(seams):
    fake = FakeLib()
    model = seams(fake)
    for bad in (torch.zeros(2, 77, 4), torch.zeros(2, 76, 8), torch.zeros(2, 77, 8, dtype=torch.float64)):
        with pytest.raises(ValueError):
            UNetContext(model, bad)
    assert fake.log == []
