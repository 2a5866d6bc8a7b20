"""The lifecycle of a native handle, written once: every Python wrapper of a network of libhedit_hip.so inherits ``NativeOwner``.

A wrapper names its C family (``_family = "dino"`` -> the ``hedit_dino_*`` entries, looked up by name) and says whether the family
has a ``finalize`` entry.  What the mix-in owns are the three attributes tests and tools read directly -- ``_h`` (a
``ctypes.c_void_p`` or None), ``_lib`` and ``_ws`` -- plus ``_h_device``, the device the handle's weights are on.  Configuration
structs, name mapping, the forward entries and what a zero workspace answer means stay in the wrappers."""
import ctypes as C

import torch

from . import _lib


# the two places the lifecycle touches the GPU runtime; a host test replaces them (and _lib._lib, _lib.cur_stream)
def _device_ctx(device):
    return torch.cuda.device(device)


def _sync_stream():
    torch.cuda.current_stream().synchronize()


class NativeOwner:
    _family = None        # "unet", "irse50", ...
    _finalizes = True     # the family has hedit_<family>_finalize (unet, vae and ddpm pack at load)
    _h = _lib = _ws = _h_device = None

    def _entry(self, lib, entry):
        return getattr(lib, f"hedit_{self._family}_{entry}")

    # ------------------------------------------------------------------ build and release
    def _native_build(self, device, params, cfg=None, create="create", after=None):
        """create -> load every parameter in the library's own order -> finalize -> ``after(lib, h)``, and only then publish
        ``_h``; a failure anywhere destroys the half-built handle and leaves ``_h`` None.  ``params``: anything indexed by
        name (a dict, a ``state_dict()``), or None to create only (the eager wrappers load later, ``_native_load``)."""
        self._native_release()
        lib = _lib.lib()
        h = C.c_void_p()
        with _device_ctx(device):
            _lib.check(self._entry(lib, create)(*(() if cfg is None else (C.byref(cfg),)), C.byref(h)))
            try:
                if params is not None:
                    self._native_upload(lib, h, device, params, self._native_param_names(lib, h))
                    if self._finalizes:
                        _lib.check(self._entry(lib, "finalize")(h, _lib.cur_stream()))
                if after is not None:
                    after(lib, h)
            except BaseException:
                self._entry(lib, "destroy")(h)
                raise
        self._h, self._lib, self._h_device = h, lib, device
        return h

    def _native_release(self):
        """destroy the handle, if there is one; safe to repeat, on an object that was never built and at interpreter shutdown"""
        try:
            h = self._h
            if h is not None:
                self._h = None
                self._entry(self._lib, "destroy")(h)
        except Exception:
            pass

    def __del__(self):
        self._native_release()

    # ------------------------------------------------------------------ parameters
    def _native_param_names(self, lib, h):
        name = self._entry(lib, "param_name")
        return [name(h, i).decode() for i in range(self._entry(lib, "num_params")(h))]

    def _native_upload(self, lib, h, device, params, names, fit=None):
        load = self._entry(lib, "load")
        for name in names:
            w = params[name] if fit is None else fit(name, params[name])
            w = w.detach().to(device=device, dtype=torch.float32).contiguous()
            _lib.check(load(h, name.encode(), _lib.ptr(w), w.numel(), _lib.cur_stream()))
            # the pack kernels are stream-ordered; keep `w` alive until they ran
            _sync_stream()

    def _native_param_shapes(self):
        """{name: shape} as the library states them, in its order"""
        shape, nd, dims, out = self._entry(self._lib, "param_shape"), C.c_int(), (C.c_int * 4)(), {}
        for i, name in enumerate(self._native_param_names(self._lib, self._h)):
            _lib.check(shape(self._h, i, C.byref(nd), dims))
            out[name] = tuple(dims[:nd.value])
        return out

    def _native_load(self, sd, strict=True, fit=None):
        """``load_state_dict`` of the eager wrappers (``self.param_shapes``, ``self.device``): the strict name check, then shape
        check and upload parameter by parameter.  ``fit(name, w)`` may reshape a tensor before its shape is checked."""
        missing = [k for k in self.param_shapes if k not in sd]
        extra = [k for k in sd if k not in self.param_shapes]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:5]} ({len(missing)}), "
                           f"unexpected {extra[:5]} ({len(extra)})")

        def checked(name, w):
            w, shape = w if fit is None else fit(name, w), self.param_shapes[name]
            if tuple(w.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(w.shape)}")
            return w

        with _device_ctx(self.device):
            self._native_upload(self._lib, self._h, self.device, sd, [k for k in self.param_shapes if k in sd], checked)
        return self

    # ------------------------------------------------------------------ workspaces
    def _grow(self, slot, need, device):
        """the buffer ``self.<slot>`` of at least ``need`` bytes on ``device``: reallocated when absent, too small or elsewhere"""
        buf, device = getattr(self, slot, None), torch.device(device)
        if (buf is None or buf.numel() < need or buf.device.type != device.type or
                (device.index is not None and buf.device.index != device.index)):
            buf = None
            setattr(self, slot, None)      # drop the old buffer before the new one exists: the peak is one buffer, not two
            buf = torch.empty(need, dtype=torch.uint8, device=device)
            setattr(self, slot, buf)
        return buf
