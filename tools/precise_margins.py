#!/usr/bin/env python3
"""The head-room table of tests/test_gpu_precise_kernels.py (profiles/precise_kernel_margins.txt): the worst error / bound ratio per
kernel and storage build, from the report the tests append to when HEDIT_MARGINS_REPORT names a file.

    HEDIT_MARGINS_REPORT=/tmp/m.tsv python -m pytest -m gpu tests/test_gpu_precise_kernels.py
    HEDIT_MARGINS_REPORT=/tmp/m.tsv HEDIT_STORAGE=f16 python -m pytest -m gpu tests/test_gpu_precise_kernels.py
    python tools/precise_margins.py /tmp/m.tsv > profiles/precise_kernel_margins.txt"""
import collections
import sys


def main(paths):
    worst = collections.OrderedDict()      # kernel -> storage -> (ratio, case, note)
    count = collections.Counter()
    for path in paths:
        for line in open(path):
            storage, what, ratio, note = (line.rstrip("\n").split("\t") + [""])[:4]
            kernel = what.split(" ")[0]
            count[(kernel, storage)] += 1
            slot = worst.setdefault(kernel, {})
            if storage not in slot or float(ratio) > slot[storage][0]:
                slot[storage] = (float(ratio), what[len(kernel):].strip(), note)
    print("worst |error| / bound per kernel (< 1 passes; the bounds are derived in tests/helpers/precise_ref.py and at each test)")
    print(f"{'kernel':20s} {'storage':7s} {'checks':>6s} {'worst':>9s}  worst case")
    for kernel, slot in worst.items():
        for storage, (ratio, case, note) in sorted(slot.items()):
            print(f"{kernel:20s} {storage:7s} {count[(kernel, storage)]:6d} {ratio:9.3f}  {case} {note}".rstrip())


if __name__ == "__main__":
    main(sys.argv[1:])
