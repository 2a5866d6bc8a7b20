"""Host: the lifecycle of a native handle (hedit/native.py NativeOwner) driven end to end with CPU tensors against a recording
fake of the library -- no GPU and no library file.  The fake stands in for ``_lib._lib``; the mix-in's two seams to the GPU runtime
(``native._device_ctx``, ``native._sync_stream``) and ``_lib.cur_stream`` are replaced.  Every entry of the fake logs
``(entry, handle)`` and can be told to raise, or to return an error code, at a chosen call."""
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib, native  # noqa: E402
from hedit.native import NativeOwner  # noqa: E402

CPU, OTHER = torch.device("cpu"), torch.device("meta")      # two devices a host has: tensors convert to both
NAMES = ["b.weight", "a.weight", "c.bias", "a.bias"]         # the library's order, not the mapping's and not sorted


class Boom(Exception):
    pass


class FakeLib:
    """hedit_<family>_{create, destroy, num_params, param_name, load, finalize}.  ``fail = (entry, k, how)``: the k-th call
    (from 1) of ``entry`` raises Boom (how = "raise") or returns -1 (how = "rc")."""

    def __init__(self, family, names, fail=None):
        self.family, self.names, self.fail = family, list(names), fail
        self.log, self.count, self.handles, self.watch = [], {}, 0, None

    def hedit_last_error(self):
        return b"fake failure"

    def __getattr__(self, name):
        prefix = f"hedit_{self.family}_"
        if not name.startswith(prefix):
            raise AttributeError(name)
        entry = name[len(prefix):]

        def call(*args):
            self.count[entry] = k = self.count.get(entry, 0) + 1
            if self.watch is not None:
                self.watch(entry)
            failing = self.fail is not None and self.fail[:2] == (entry, k)
            if failing and self.fail[2] == "raise":
                raise Boom(f"{entry} #{k}")
            if entry == "create":
                if failing:
                    return -1
                self.handles += 1
                args[-1]._obj.value = 0x1000 * self.handles
                self.log.append(("create", args[-1]._obj.value))
                return 0
            h = args[0].value
            if entry == "num_params":
                return len(self.names)
            if entry == "param_name":
                return self.names[args[1]].encode()
            self.log.append((entry, h) if entry != "load" else (entry, h, args[1].decode(), args[3]))
            return -1 if failing else (None if entry == "destroy" else 0)
        return call


class Owner(NativeOwner):
    _family = "toy"


def params():
    return {n: torch.full((i + 1, 2), float(i)) for i, n in enumerate(sorted(NAMES))}


@pytest.fixture
def seams(monkeypatch):
    monkeypatch.setattr(native, "_device_ctx", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(native, "_sync_stream", lambda: None)
    monkeypatch.setattr(_lib, "cur_stream", lambda: None)

    def install(fake):
        monkeypatch.setattr(_lib, "_lib", fake)
        return fake
    return install


def full_build(h, names, p):
    return [("create", h)] + [("load", h, n, p[n].numel()) for n in names] + [("finalize", h)]


def test_build_runs_create_loads_finalize_and_only_then_publishes(seams):
    fake, o, p, seen = seams(FakeLib("toy", NAMES)), Owner(), params(), []
    fake.watch = lambda entry: seen.append((entry, o._h))
    after = []
    h = o._native_build(CPU, p, after=lambda lib, hh: after.append((lib, hh.value, o._h)))
    assert fake.log == full_build(0x1000, NAMES, p)
    assert [e for e, _ in seen if e in ("create", "load", "finalize")] == ["create"] + ["load"] * 4 + ["finalize"]
    assert all(published is None for _, published in seen) and after == [(fake, 0x1000, None)]
    assert o._h is h and h.value == 0x1000 and o._lib is fake and o._h_device == CPU


def test_a_family_without_finalize_and_a_create_variant(seams):
    class Eager(NativeOwner):
        _family, _finalizes = "toy", False
    fake, o, p = seams(FakeLib("toy", NAMES)), Eager(), params()
    cfg = _lib.VitCfg(1, 2, 3, 4, 5)
    o._native_build(CPU, p, cfg)
    assert fake.log == full_build(0x1000, NAMES, p)[:-1]
    fake.log.clear()
    o._native_build(CPU, None, cfg, create="create")          # create only: what the eager wrappers do at construction
    assert fake.log == [("destroy", 0x1000), ("create", 0x2000)] and o._h.value == 0x2000


@pytest.mark.parametrize("fail,error", [(("create", 1, "raise"), Boom), (("create", 1, "rc"), _lib.HipError),
                                        (("load", 1, "raise"), Boom), (("load", 3, "raise"), Boom), (("load", 2, "rc"), _lib.HipError),
                                        (("finalize", 1, "raise"), Boom), (("finalize", 1, "rc"), _lib.HipError)])
def test_a_failed_build_destroys_what_it_created_and_publishes_nothing(seams, fail, error):
    fake, o, p = seams(FakeLib("toy", NAMES, fail)), Owner(), params()
    with pytest.raises(error) as e:
        o._native_build(CPU, p)
    if error is Boom:
        assert e.value.args == (f"{fail[0]} #{fail[1]}",)          # the exception itself, not a wrapped one
    destroys = [x for x in fake.log if x[0] == "destroy"]
    assert destroys == ([] if fail[0] == "create" else [("destroy", 0x1000)]) and fake.log[-1:] == destroys[-1:]
    assert o._h is None
    fake.fail, n = None, len(fake.log)
    o._native_build(CPU, p)
    h = o._h.value
    assert fake.log[n:] == full_build(h, NAMES, p) and h == (0x1000 if fail[0] == "create" else 0x2000)


def test_a_missing_parameter_is_a_key_error_and_leaves_nothing_behind(seams):
    fake, o, p = seams(FakeLib("toy", NAMES)), Owner(), params()
    del p["c.bias"]
    with pytest.raises(KeyError) as e:
        o._native_build(CPU, p)
    assert e.value.args == ("c.bias",)
    assert fake.log == full_build(0x1000, NAMES[:2], p)[:-1] + [("destroy", 0x1000)] and o._h is None
    o._native_build(CPU, params())
    assert fake.log[-6:] == full_build(0x2000, NAMES, params())


def test_release_is_idempotent_and_silent_on_an_owner_never_built(seams):
    fake, o = seams(FakeLib("toy", NAMES)), Owner()
    o._native_release()
    o.__del__()
    Owner.__new__(Owner).__del__()
    assert fake.log == [] and fake.count == {}
    o._native_build(CPU, params())
    fake.log.clear()
    o._native_release()
    o._native_release()
    o.__del__()
    assert fake.log == [("destroy", 0x1000)] and o._h is None
    o._native_build(CPU, params())
    fake.fail = ("destroy", 2, "raise")                  # a library that is being torn down: release stays silent
    o.__del__()
    assert o._h is None


def test_a_second_device_destroys_the_old_handle_and_creates_anew(seams):
    class Lazy(Owner):
        def _native(self, device):
            if self._h is None or self._h_device != device:
                self._native_build(device, params())
            return self._h
    fake, o = seams(FakeLib("toy", NAMES)), Lazy()
    assert o._native(CPU).value == 0x1000 and o._native(CPU).value == 0x1000 and fake.count["create"] == 1
    fake.log.clear()
    assert o._native(OTHER).value == 0x2000 and o._h_device == OTHER
    assert fake.log[:2] == [("destroy", 0x1000), ("create", 0x2000)] and fake.log == fake.log[:1] + full_build(0x2000, NAMES, params())


def test_grow_keeps_a_buffer_that_is_large_enough():
    o = Owner()
    a = o._grow("_ws", 100, CPU)
    assert a.dtype == torch.uint8 and a.numel() == 100 and o._ws is a
    assert o._grow("_ws", 100, CPU) is a and o._grow("_ws", 7, "cpu").data_ptr() == a.data_ptr()
    b = o._grow("_ws", 101, CPU)
    assert b is not a and b.numel() == 101 and o._ws is b
    c = o._grow("_ws", 5, OTHER)
    assert c.device == OTHER and c.numel() == 5 and o._ws is c
    assert o._grow("_gws", 3, CPU) is o._gws and o._ws is c          # slots are independent


# ---------------------------------------------------------------------------------------------- two real wrappers
def test_face_parsing_publishes_no_half_built_handle(seams):
    """the regression: a build that failed after ``create`` used to leave ``_h`` set, and the next call returned that
    never-finalized handle"""
    from hedit.arcface import FaceParsing
    net = FaceParsing().init_random(0)
    names = list(net.param_shapes)
    fake = seams(FakeLib("faceparse", names, ("load", 3, "raise")))
    with pytest.raises(Boom):
        net._native(CPU)
    assert net._h is None and fake.log[-1] == ("destroy", 0x1000)
    healthy = seams(FakeLib("faceparse", names))
    h = net._native(CPU)
    sd = net.state_dict()
    assert healthy.log == full_build(h.value, names, sd) and net._h is h
    assert net._native(CPU) is h and healthy.count["create"] == 1
    net.reset_native()
    assert net._h is None and healthy.log[-1] == ("destroy", h.value)


def test_a_clip_sibling_follows_its_parent(seams):
    from hedit.clip_guidance.base_clip import CLIPEncoder, ClipVisualPrefix
    enc = CLIPEncoder(clip_model=ClipVisualPrefix(width=64, layers=1, heads=1, patch_size=16, input_resolution=32).init_random(0))
    fake = seams(FakeLib("vit", list(enc.clip_model.state_dict())))
    sib = enc.sibling(torch.zeros(1, 3, 32, 32))
    assert sib._h is None                                     # nothing built yet: nothing to share
    first = enc._native(CPU).value
    assert sib._h.value == first and sib._lib is fake and sib._width == enc._width == 64
    assert sib._native(CPU).value == first and fake.count["create"] == 1
    second = sib._native(OTHER).value                         # asked through the sibling: the PARENT rebuilds
    assert second != first and enc._h.value == second and sib._h.value == second and enc._h_device == OTHER
    assert fake.log.index(("destroy", first)) + 1 == fake.log.index(("create", second))
    n = len(fake.log)
    sib.__del__()
    assert fake.log[n:] == [] and enc._h.value == second     # a sibling owns nothing
    enc._native_release()
    assert fake.log[n:] == [("destroy", second)] and sib._h is None
