"""ms to build the SD-1.5-shaped UNet handle: hedit_unet_create, hedit_unet_load of every parameter (weights already on the
device, one synchronisation at the end) and the first hedit_unet_workspace_bytes.  `python tools/unet_build_time.py [builds]`"""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
from hedit import _lib  # noqa: E402
if os.environ.get("HEDIT_LIB_VARIANT"):       # tools/build_variant.sh side library (A/B runs inside one GPU call)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"lib_{os.environ['HEDIT_LIB_VARIANT']}.so.bin")
from hedit.unet import SD15_CONFIG, UNet2DConditionModel  # noqa: E402


def main():
    builds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lib = _lib.lib()
    probe = UNet2DConditionModel(dict(SD15_CONFIG), device="cuda:0")
    cfg, g = probe._cfg_struct, torch.Generator().manual_seed(3)
    sd = [(k.encode(), (torch.randn(*s, generator=g) * 0.02).cuda()) for k, s in probe.param_shapes.items()]
    probe._native_release()
    torch.cuda.synchronize()
    rows = []
    for _ in range(builds):
        h = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.hedit_unet_create(C.byref(cfg), C.byref(h)))
        t1 = time.perf_counter()
        for name, w in sd:
            _lib.check(lib.hedit_unet_load(h, name, _lib.ptr(w), w.numel(), _lib.cur_stream()))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        need = lib.hedit_unet_workspace_bytes(h, 2, 64, 64)
        t3 = time.perf_counter()
        assert need > 0 and lib.hedit_unet_missing(h) == 0
        lib.hedit_unet_destroy(h)
        rows.append([round((b - a) * 1e3, 2) for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))])
    print(f"unet build, {len(sd)} parameters, ms per build [create, load, workspace_bytes, total]: {rows}", flush=True)


if __name__ == "__main__":
    main()
