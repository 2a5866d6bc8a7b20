"""-m gpu: the handle lifecycle of hedit/native.py on the real library, through three lazily built wrappers at the smallest
configurations their own test files use (tests/test_gpu_text.py's stand-in for the tiny UNet, the 26-token case of
tests/test_gpu_dino.py, tests/test_gpu_face_parsing.py's network on a 32 x 32 image).  Release and rebuild, and a build that
fails on the host half way (a name missing from the parameter mapping: KeyError, nothing faulty reaches the device), must leave
no handle behind and must not change a bit of the next result -- same weights, same kernels, and the executors do not depend on
history.  Every comparison is ``torch.equal``."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from helpers import gpu as G  # noqa: E402
from helpers import dino_ref as DR  # noqa: E402
from helpers.parsing import parsing_state_dict  # noqa: E402


def _text():
    from hedit.text import ClipTextEncoder, NativeClipText
    from hedit.unet import TINY_CONFIG
    enc = NativeClipText.from_standin(ClipTextEncoder(dim=TINY_CONFIG["cross_attention_dim"], layers=2, heads=1, seed=7), device=G.dev())
    ids = torch.tensor([[49406, 5, 17, 230, 49407] + [49407] * 72, [49406, 9, 49407] + [49407] * 74])

    def swap(params):
        old, enc.params = enc.params, params
        return old
    return enc, (lambda: enc(ids)[0]), (lambda: enc.params), swap


def _dino():
    from hedit.dino_score import NativeDinoStructure
    m = NativeDinoStructure(DR.net_of("t26"), device=G.dev())
    a, b = (t.to(G.dev()) for t in DR.parity_inputs("t26"))

    def swap(params):
        old, m.net.params = m.net.params, params
        return old
    return m, (lambda: m.distance(a, b)), (lambda: m.net.params), swap


def _faceparse():
    from hedit.arcface import FaceParsing
    meta = json.load(open(os.path.join(HERE, "golden", "g17_face_parsing.json")))
    net = FaceParsing(device="cuda:0")
    net.load_state_dict(parsing_state_dict({k: tuple(s) for k, s in meta["params"]}))
    x = (torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    real = net.state_dict

    def swap(params):
        net.state_dict = real if params is None else (lambda: params)
    return net, (lambda: net(x)), real, swap


@pytest.mark.parametrize("make", [_text, _dino, _faceparse])
def test_release_rebuild_and_a_failed_build_leave_the_bits_alone(make):
    owner, evaluate, params, swap = make()
    assert owner._h is None                      # built on first use
    first = evaluate().clone()
    assert owner._h is not None and owner._h.value
    owner._native_release()
    assert owner._h is None
    again = evaluate()
    assert owner._h is not None and torch.equal(again, first)
    owner._native_release()
    good = dict(params())
    old = swap({k: v for k, v in good.items() if k != list(good)[-1]})
    with pytest.raises(KeyError):
        evaluate()
    assert owner._h is None
    swap(old)
    restored = evaluate()
    G.sync()
    assert owner._h is not None and torch.equal(restored, first)
