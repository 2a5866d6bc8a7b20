"""CPU: bench.py --dump-outputs writes float32 arrays inside its 64 MB budget; an output over its share becomes a seeded sample of
its elements, the same one on every call (tests/test_gpu_bench.py runs the flag end to end on the GPU)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_budget_and_sample(tmp_path):
    big = torch.arange(600 * 4 * 64 * 64, dtype=torch.float64).reshape(600, 4, 64, 64)    # 37.5 MB as float32: over half the budget
    small = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["big.npy", "small.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= bench.DUMP_BUDGET_BYTES
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())
    b = np.load(tmp_path / "a" / "big.npy")
    # the elements are their own flat indices: a sample of distinct indices in ascending order
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_BUDGET_BYTES // 2 // 4,)
    assert (np.diff(b) > 0).all() and b[0] >= 0 and b[-1] < big.numel()
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))


def test_dump_outputs_other_ranks(tmp_path):
    x = torch.ones(2, 3)
    bench.dump_outputs(str(tmp_path), {"edit": x}, rank=1, world=2)
    assert os.listdir(tmp_path) == ["edit_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "edit_rank1.npy"), x.numpy())
