"""-m gpu: hedit_attn_aggregate (csrc/step.hip) through the C ABI -- the reduction behind aggregate_attention.

Accuracy is checked against an fp64 restatement of the definition in include/hedit.h with the derived elementwise bound
(n_maps * heads + 2) * 2^-24 * sum|terms| / (n_maps * heads): a left-to-right fp32 sum of n_maps * heads terms plus the two
divisions (tests/helpers/p2p_generate_ref.py::kernel_ref64).  Batch invariance, repeatability, the scalar path and the
untouched guard bands are exact comparisons."""
import ctypes as C

import pytest
import torch

from helpers import gpu as G
from helpers import p2p_generate_ref as PR
from hedit import _lib

pytestmark = pytest.mark.gpu


def _aggregate(maps, cur_step, out=None, stream=None):
    n_img, _, heads, tokens, cols = maps[0].shape
    if out is None:
        out = torch.empty(n_img, 2, tokens, cols, dtype=torch.float32, device=maps[0].device)
    arr = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    _lib.check(_lib.lib().hedit_attn_aggregate(arr, len(maps), heads, tokens, cols, n_img, cur_step, _lib.ptr(out), stream))
    G.sync()
    return out


def _maps(seed, n_maps, n_img, heads, tokens, cols):
    g = torch.Generator(device=G.dev()).manual_seed(seed)
    return [torch.rand(n_img, 2, heads, tokens, cols, generator=g, device=G.dev()) for _ in range(n_maps)]


def _check(maps, cur_step, out):
    want, bound = PR.kernel_ref64(maps, cur_step)
    err = (out.double() - want).abs()
    ratio = (err / bound).max().item()
    print(f"maps {len(maps)} x {tuple(maps[0].shape)} cur_step {cur_step}: max |err| {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(out).all() and (err <= bound).all()


@pytest.mark.parametrize("cur_step", [1, 7])
@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("n_maps", [1, 3, 5])
@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("tokens", [64, 256])
@pytest.mark.parametrize("heads", [1, 8])
def test_attn_aggregate_matches_fp64_and_is_batch_invariant(heads, tokens, cross, n_maps, n_img, cur_step):
    cols = 77 if cross else tokens
    maps = _maps(1000 * heads + tokens + n_maps + 10 * n_img + cur_step, n_maps, n_img, heads, tokens, cols)
    out = _aggregate(maps, cur_step)
    _check(maps, cur_step, out)
    assert torch.equal(_aggregate(maps, cur_step), out)                      # a second run
    for i in range(n_img if n_img > 1 else 0):                               # image i alone: the bits of its batch row
        alone = _aggregate([m[i:i + 1].contiguous() for m in maps], cur_step)
        assert torch.equal(alone[0], out[i])


def test_attn_aggregate_at_1024_tokens():
    maps = _maps(5, 1, 1, 8, 1024, 1024)
    out = _aggregate(maps, 3)
    _check(maps, 3, out)
    assert torch.equal(_aggregate(maps, 3), out)


@pytest.mark.parametrize("tokens,cols,lead", [(64, 77, 64), (64, 77, 1), (9, 77, 64), (9, 77, 3), (5, 5, 2)])
def test_attn_aggregate_leaves_the_guard_bands_alone(tokens, cols, lead):
    """out inside a NaN-filled buffer.  lead = 64 floats keeps it 16-byte aligned (the 128-bit path where tokens * cols is a
    multiple of 4), the odd leads and 9 x 77 = 693 elements take the scalar path: the same bits, nothing written outside
    [n_img][2][tokens][cols]."""
    n_img, heads, cur_step = 2, 3, 4
    maps = _maps(tokens + lead, 2, n_img, heads, tokens, cols)
    size = n_img * 2 * tokens * cols
    buf = torch.full((lead + size + 64,), float("nan"), dtype=torch.float32, device=G.dev())
    out = buf[lead:lead + size].view(n_img, 2, tokens, cols)
    _aggregate(maps, cur_step, out=out)
    assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + size:]).all()
    _check(maps, cur_step, out)
    assert torch.equal(out, _aggregate(maps, cur_step))                      # an aligned buffer of its own: the same bits


def test_attn_aggregate_refuses_bad_arguments_before_launching():
    lib = _lib.lib()
    maps = _maps(1, 2, 1, 2, 16, 77)
    out = torch.full((1, 2, 16, 77), float("nan"), dtype=torch.float32, device=G.dev())
    arr = (C.c_void_p * 2)(*[m.data_ptr() for m in maps])
    holed = (C.c_void_p * 2)(maps[0].data_ptr(), None)
    o = _lib.ptr(out)
    #        h_maps n_maps heads tokens cols n_img cur_step out   what the message names
    bad = [(arr, 0, 2, 16, 77, 1, 3, o, "n_maps"), (arr, 17, 2, 16, 77, 1, 3, o, "16 maps"), (arr, 2, 2, 16, 77, 1, 0, o, "cur_step"),
           (arr, 2, 0, 16, 77, 1, 3, o, "heads"), (arr, 2, 2, 16, 0, 1, 3, o, "cols"), (arr, 2, 2, 0, 77, 1, 3, o, "tokens"),
           (arr, 2, 2, 16, 77, 0, 3, o, "n_img"), (None, 2, 2, 16, 77, 1, 3, o, "h_maps"), (arr, 2, 2, 16, 77, 1, 3, None, "out"),
           (holed, 2, 2, 16, 77, 1, 3, o, "null map")]
    for *args, what in bad:
        rc = lib.hedit_attn_aggregate(*args, None)
        assert rc != 0, what
        assert what in lib.hedit_last_error().decode(), (what, lib.hedit_last_error().decode())
    G.sync()
    assert torch.isnan(out).all()                                            # nothing was launched
    _check(maps, 3, _aggregate(maps, 3, out=out))
