"""-m gpu: a bound text context (hedit_unet_context, UNet2DConditionModel.make_context).  The object holds what every
hedit_unet_forward call computes first from its context rows -- the padded bf16 rows and the attn2 key / value projections of all
transformer blocks -- made once by the same launches, so a call that is handed the object gives the BITS of the call that is handed
the tensor: plain, over shared latents, and under a P2P plan.  It is a snapshot (the tensor may change afterwards), it is tied to
its handle and its row count (HEDIT_ERR_ARG otherwise), and it may be destroyed before or after the model."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import gpu as G  # noqa: E402
from helpers.models import make_hip  # noqa: E402
from helpers.tiny import PROMPT_PAIRS  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.unet import TINY_CONFIG, UNet2DConditionModel  # noqa: E402


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_hip(TINY_CONFIG, 4)


def _inputs(D, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(D, 4, 32, 32, generator=g)
    ctx = torch.randn(B, 77, TINY_CONFIG["cross_attention_dim"], generator=g)
    return G.f32(x), G.f32(ctx)


def _batch_controller(hip, pairs, T):
    from hedit.p2p import ptp_controller_utils as PCU
    from hedit.p2p.ptp_classes import ControllerBatch
    from hedit.p2p.ptp_utils import register_attention_control
    ctrls = [PCU.make_controller(prompts=[s_, t_], is_replace_controller=is_replace, cross_replace_steps=0.4, self_replace_steps=0.35,
                                 blend_word=((bw[0],), (bw[1],)), equilizer_params={"words": (bw[1],), "values": (2.0,)},
                                 num_steps=T, tokenizer=hip.tokenizer, device=hip.device) for (s_, t_, bw, is_replace) in pairs]
    cb = ControllerBatch(ctrls)
    register_attention_control(hip, cb)
    return cb


def _unregister(hip):
    from hedit.unet import AttnProcessor
    hip.unet.set_attn_processor({k: AttnProcessor() for k in hip.unet.attn_processors})


def test_plain_call(tiny):
    unet = tiny.unet
    x, ctx = _inputs(4, 4, 1)
    want = unet.forward_raw(x, 401.0, ctx)
    cx = unet.make_context(ctx)
    got = unet.forward_raw(x, 401.0, cx)
    G.sync()
    assert cx.rows == 4 and torch.isfinite(want).all()
    assert torch.equal(got, want)
    cx.close()
    cx.close()                      # safe to repeat
    with pytest.raises(_lib.HipError):
        unet.forward_raw(x, 401.0, cx)


def test_shared_latents_call(tiny):
    """5 rows over 2 latents: the stem runs once per latent (hedit_unet_forward_shared_bound)"""
    unet = tiny.unet
    rmap = [0, 1, 0, 1, 1]
    x, ctx = _inputs(2, 5, 2)
    want = unet.forward_raw(x, 401.0, ctx, row_latent=rmap)
    rows = unet.forward_raw(x[rmap].contiguous(), 401.0, ctx)
    cx = unet.make_context(ctx)
    got = unet.forward_raw(x, 401.0, cx, row_latent=rmap)
    G.sync()
    assert torch.equal(got, want) and torch.equal(got, rows)


def test_call_under_a_p2p_plan(tiny):
    x, ctx = _inputs(4, 4, 3)
    try:
        cb = _batch_controller(tiny, [PROMPT_PAIRS[0]], 4)
        plan = cb._plan(tiny.unet, 4, 32, 32, True)
        want = tiny.unet.forward_raw(x, 401.0, ctx, plan)
        cx = tiny.unet.make_context(ctx)
        got = tiny.unet.forward_raw(x, 401.0, cx, plan)
        G.sync()
    finally:
        _unregister(tiny)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)


def test_two_contexts_alive_and_used_alternately(tiny):
    unet = tiny.unet
    x, ctx_a = _inputs(4, 4, 4)
    x2, ctx_b = _inputs(2, 2, 5)
    want_a, want_b = unet.forward_raw(x, 301.0, ctx_a), unet.forward_raw(x2, 301.0, ctx_b)
    cx_a, cx_b = unet.make_context(ctx_a), unet.make_context(ctx_b)
    for _ in range(2):
        assert torch.equal(unet.forward_raw(x, 301.0, cx_a), want_a)
        assert torch.equal(unet.forward_raw(x2, 301.0, cx_b), want_b)
    G.sync()


def test_the_context_is_a_snapshot(tiny):
    unet = tiny.unet
    x, ctx = _inputs(4, 4, 6)
    old = unet.forward_raw(x, 401.0, ctx)
    cx = unet.make_context(ctx)
    ctx.mul_(-0.5).add_(0.25)
    G.sync()
    new = unet.forward_raw(x, 401.0, ctx)
    G.sync()
    assert not torch.equal(new, old)
    assert torch.equal(unet.forward_raw(x, 401.0, cx), old)
    assert torch.equal(unet.forward_raw(x, 401.0, unet.make_context(ctx)), new)


def test_wrong_rows_and_wrong_handle_are_argument_errors(tiny):
    unet = tiny.unet
    x, ctx = _inputs(4, 4, 7)
    cx = unet.make_context(ctx)
    with pytest.raises(_lib.HipError, match="error -1"):
        unet.forward_raw(x[:2].contiguous(), 401.0, cx)
    with pytest.raises(_lib.HipError, match="error -1"):
        unet.forward_raw(x[:2].contiguous(), 401.0, cx, row_latent=[0, 1, 0])
    other = UNet2DConditionModel(TINY_CONFIG, device=G.dev())
    other.init_random(5)
    with pytest.raises(_lib.HipError, match="error -1"):
        other.forward_raw(x, 401.0, cx)
    G.sync()
    assert torch.isfinite(unet.forward_raw(x, 401.0, cx)).all()


def test_destroy_before_and_after_the_model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    model = UNet2DConditionModel(TINY_CONFIG, device=G.dev())
    model.init_random(2)
    x, ctx = _inputs(4, 4, 8)
    first, second = model.make_context(ctx), model.make_context(ctx)
    want = model.forward_raw(x, 401.0, ctx)
    assert torch.equal(model.forward_raw(x, 401.0, first), want)
    G.sync()
    first.close()                   # before the model
    assert first._h is None
    model._native_release()
    second.close()                  # after it
    assert second._h is None
    G.sync()


def test_engine_run_with_and_without_bound_contexts(tiny):
    """3 steps, 2 images, P2P + LocalBlend, the 5n-row pass: edit and reconstruction keep their bits"""
    from hedit.engine import HEditEngine
    T, n = 3, 2
    tiny.scheduler.set_timesteps(T)
    try:
        pairs = [PROMPT_PAIRS[i % len(PROMPT_PAIRS)] for i in range(n)]
        prompt_pairs = [[p[0], p[1]] for p in pairs]
        w0 = torch.stack([torch.randn(4, 32, 32, generator=torch.Generator().manual_seed(40 + i)) * 0.8 for i in range(n)]).to(G.dev())
        gen = torch.Generator(device=G.dev()).manual_seed(9)
        zs, xts = HEditEngine(tiny).ddpm_inversion(w0, [p[0] for p in prompt_pairs], eta=1.0, cfg_src=1.0, generator=gen)
        outs = []
        for bind in (True, False):
            cb = _batch_controller(tiny, pairs, T)
            eng = HEditEngine(tiny)
            eng._bind_contexts = bind
            made = []
            real = tiny.unet.make_context
            tiny.unet.make_context = lambda rows: made.append(real(rows)) or made[-1]
            try:
                outs.append(eng.run(xts[T].contiguous(), zs, prompt_pairs, [1.0, 5.0, 7.5], cb, eta=1.0, p2p=True, implicit=True, K=1,
                                    w_rec=0.1, after_skip_steps=T, ddim_inv=False, fuse_src_pass=True))
            finally:
                del tiny.unet.make_context
            G.sync()
            assert len(made) == (2 if bind else 0)              # base4 and edit5, each once
            assert all(cx._h is None for cx in made)            # dropped on return
    finally:
        _unregister(tiny)
        tiny.scheduler.set_timesteps(4)
    (e1, r1), (e0, r0) = outs
    assert torch.isfinite(e1).all()
    assert torch.equal(e1, e0) and torch.equal(r1, r0)
    assert torch.equal(r1, xts[0])
