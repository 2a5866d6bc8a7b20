"""The one-launch GroupNorm of the 16 x 16 and 8 x 8 levels (csrc/norm.hip: gn_small_kernel) at the six shapes one UNet call
runs it at, `python tools/gn_small_bench.py [rows ...]` (default 120 96).  Per shape: median / min of 24 event-timed launches
after warm-up, each on another (x, y) pair of a pool larger than the 256 MB Infinity Cache, and the rate at which the
4 B per element (one read, one write) move.  On a library that has hedit_test_set_flags bit 4 the kept narrow kernel is
timed next to the product kernel, launch by launch alternating, and the outputs are compared with torch.equal.
`--few` = 3 launches per shape and variant, no timing table (for a counter pass under rocprofv3 --pmc)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
import torch  # noqa: E402
from hedit import _lib  # noqa: E402

SHAPES = [(256, 1280, 11), (256, 2560, 2), (256, 1920, 1), (256, 640, 1), (64, 1280, 12), (64, 2560, 3)]   # (HW, C, launches per call)
POOL_BYTES = 640 << 20


def main():
    few = "--few" in sys.argv
    rows = [int(a) for a in sys.argv[1:] if a.isdigit()] or [120, 96]
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    has_ref = lib.hedit_test_set_flags(16) == 0
    lib.hedit_test_set_flags(0)
    variants = [("product", 0)] + ([("kept", 16)] if has_ref else [])
    n_timed = 3 if few else 24
    print(f"storage {_lib.STORAGE}; variants {[v for v, _ in variants]}; {n_timed} launches per shape and variant")
    for B in rows:
        total = {v: 0.0 for v, _ in variants}
        for hw, c, per_call in SHAPES:
            elems = B * hw * c
            npair = max(2, min(8, POOL_BYTES // (elems * 4) + 1))
            gen = torch.Generator(device=dev).manual_seed(hw + c)
            xs = [(torch.randn(B * hw, c, device=dev, generator=gen) * 2 + 0.5).to(_lib.storage_dtype()) for _ in range(npair)]
            ys = {v: [torch.empty_like(x) for x in xs] for v, _ in variants}
            g = 1 + 0.1 * torch.randn(c, device=dev, generator=gen)
            b = 0.1 * torch.randn(c, device=dev, generator=gen)
            ws = torch.empty(max(lib.hedit_k_groupnorm_ws_bytes(B, hw, c), 16), dtype=torch.uint8, device=dev)
            times = {v: [] for v, _ in variants}

            def launch(v, flags, i):
                if has_ref:
                    _lib.check(lib.hedit_test_set_flags(flags))
                _lib.check(lib.hedit_k_groupnorm(_lib.ptr(xs[i]), _lib.ptr(ys[v][i]), _lib.ptr(g), _lib.ptr(b), B, hw, c, 32, 1e-5, 1,
                                                 _lib.ptr(ws), None))

            try:
                for i in range(npair):                       # warm-up: every buffer, every variant
                    for v, flags in variants:
                        launch(v, flags, i)
                torch.cuda.synchronize()
                for it in range(n_timed):
                    for v, flags in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        launch(v, flags, it % npair)
                        e1.record()
                        e1.synchronize()
                        times[v].append(e0.elapsed_time(e1) * 1e3)
            finally:
                if has_ref:
                    lib.hedit_test_set_flags(0)
            same = all(torch.equal(ys["product"][i], ys["kept"][i]) for i in range(npair)) if has_ref else None
            line = f"rows={B:4d} HW={hw:4d} C={c:5d} x{per_call:2d}"
            for v, _ in variants:
                med = statistics.median(times[v])
                total[v] += med * per_call
                line += f" | {v}: median {med:7.1f} us (min {min(times[v]):7.1f})  {elems * 4 / med / 1e6:5.2f} TB/s"
            if same is not None:
                line += f" | torch.equal {same}"
            print(line, flush=True)
            del xs, ys
        print(f"rows={B:4d} sum over the 30 launches of a call: " + ", ".join(f"{v} {total[v] / 1e3:.3f} ms" for v, _ in variants), flush=True)


if __name__ == "__main__":
    main()
