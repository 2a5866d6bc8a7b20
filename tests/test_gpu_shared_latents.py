"""-m gpu: one UNet call over rows that share latents (hedit_unet_forward_shared, forward_raw(row_latent=)).

Classifier-free guidance and the h-Edit passes evaluate each latent under several contexts in one batch.  Until the
first cross-attention a row's activations depend on its latent and the timestep only, and the kernels are bitwise batch
invariant (test_gpu_invariance.py), so running that part once per DISTINCT latent is a common-subexpression elimination:
every assertion here is BIT equality against the call on the materialised rows -- for any row map, under a P2P plan where
the plan leaves the first block alone, and through the fall-back (latents spread to one per row first) where it does not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import gpu as G  # noqa: E402
from helpers.models import make_hip  # noqa: E402
from helpers.tiny import PROMPT_PAIRS  # noqa: E402
from hedit.unet import SD15_CONFIG, TINY_CONFIG  # noqa: E402

# SD-1.x's block layout at toy widths: fed 64 x 64 latents its first transformer block has 4096 tokens (no self-replace, no
# stored maps there, so a P2P plan leaves the shared part alone) and LocalBlend finds its 16 x 16 cross maps
TINY4_CONFIG = dict(TINY_CONFIG, sample_size=64, block_out_channels=(64, 128, 128, 128),
                    down_block_types=SD15_CONFIG["down_block_types"], up_block_types=SD15_CONFIG["up_block_types"])


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    _need_gpu()
    return make_hip(TINY_CONFIG, 4)


@pytest.fixture(scope="module")
def tiny4():
    _need_gpu()
    return make_hip(TINY4_CONFIG, 4, seed=1)


@pytest.fixture(scope="module")
def sd15():
    _need_gpu()
    return make_hip(SD15_CONFIG, 10, seed=3)


def _inputs(D, B, cfg, size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(D, 4, size, size, generator=g)
    ctx = torch.randn(B, 77, cfg["cross_attention_dim"], generator=g)      # a context of its own for every row
    return G.f32(x), G.f32(ctx)


def _shared_vs_rows(unet, x, ctx, rmap, t, plan=None, exact_ws=False):
    want = unet.forward_raw(x[rmap].contiguous(), t, ctx, plan)
    G.sync()
    if exact_ws:
        unet._ws = None          # the next call allocates exactly hedit_unet_workspace_bytes(B, H, W)
    got = unet.forward_raw(x, t, ctx, plan, row_latent=rmap)
    G.sync()
    if exact_ws:
        assert unet._ws.numel() == unet._lib.hedit_unet_workspace_bytes(unet._h, len(rmap), x.shape[2], x.shape[3])
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)


TINY_MAPS = [(3, [0, 1, 2, 0, 1, 2, 0, 2], True), (3, [2, 0, 2, 1], False), (3, [0, 1, 2], False), (1, [0, 0, 0, 0], False)]


@pytest.mark.parametrize("D,rmap,exact_ws", TINY_MAPS, ids=["interleaved-exact-workspace", "unsorted", "identity", "one-latent"])
def test_tiny_rows_of_a_map_equal_the_materialised_rows(tiny, D, rmap, exact_ws):
    unet = tiny.unet
    x, ctx = _inputs(D, len(rmap), TINY_CONFIG, 32, 11 + len(rmap))
    _shared_vs_rows(unet, x, ctx, rmap, 401.0, exact_ws=exact_ws)


def test_tiny_shared_part_really_runs_once_per_latent(tiny):
    """the sampled launch records say what ran: the first GEMM launches at D * HW rows, the gather under `other`, the head at B * HW"""
    unet = tiny.unet
    rmap = [0, 1, 2, 0, 1, 2, 0, 2]
    x, ctx = _inputs(3, len(rmap), TINY_CONFIG, 32, 5)
    unet.prof_reset()
    unet.prof_enable(True, 4096)
    try:
        unet.forward_raw(x, 401.0, ctx, row_latent=rmap)
        rec = unet.prof_records()
    finally:
        unet.prof_enable(False, 4096)
        unet.prof_reset()
    gemm = rec[(rec[:, 0] == 0) | (rec[:, 0] == 1)]
    m = [int(v) for v in gemm[:, 4]]
    assert 3 * 1024 in m and 8 * 1024 in m
    first_conv = rec[rec[:, 0] == 0][0]
    assert int(first_conv[4]) == 3 * 1024
    assert (rec[:, 0] == 5).sum() >= 1


def test_bad_maps_are_refused(tiny):
    from hedit import _lib
    unet = tiny.unet
    x, ctx = _inputs(2, 3, TINY_CONFIG, 32, 2)
    for bad in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(_lib.HipError):
            unet.forward_raw(x, 401.0, ctx, row_latent=bad)
    G.sync()


def _batch_controller(hip, pairs, T, K):
    from hedit.p2p import ptp_controller_utils as PCU
    from hedit.p2p.ptp_classes import ControllerBatch
    from hedit.p2p.ptp_utils import register_attention_control
    ctrls = []
    for (s_, t_, bw, is_replace) in pairs:
        ctrls.append(PCU.make_controller(prompts=[s_, t_], is_replace_controller=is_replace, cross_replace_steps=0.4,
                                         self_replace_steps=0.35, blend_word=((bw[0],), (bw[1],)),
                                         equilizer_params={"words": (bw[1],), "values": (2.0 if K == 1 else 1.25,)},
                                         num_steps=T, tokenizer=hip.tokenizer, device=hip.device))
    cb = ControllerBatch(ctrls)
    register_attention_control(hip, cb)
    return cb


def _unregister(hip):
    from hedit.unet import AttnProcessor
    hip.unet.set_attn_processor({k: AttnProcessor() for k in hip.unet.attn_processors})


def _loop_both_ways(hip, size, n, T, K, fuse, seed):
    """inversion + P2P / LocalBlend loop with share_latents on and off, on the same inversion: [(edit, recon, maps)] * 2, xts"""
    from hedit.engine import HEditEngine
    hip.scheduler.set_timesteps(T)
    pairs = [PROMPT_PAIRS[i % len(PROMPT_PAIRS)] for i in range(n)]
    prompt_pairs = [[p[0], p[1]] for p in pairs]
    w0 = torch.stack([torch.randn(4, size, size, generator=torch.Generator().manual_seed(seed + i)) * 0.8 for i in range(n)]).to(G.dev())
    inv = []
    for share in (True, False):
        gen = torch.Generator(device=G.dev()).manual_seed(seed)
        inv.append(HEditEngine(hip, share_latents=share).ddpm_inversion(w0, [p[0] for p in prompt_pairs], eta=1.0, cfg_src=1.0, generator=gen))
    G.sync()
    assert torch.equal(inv[0][0], inv[1][0]) and torch.equal(inv[0][1], inv[1][1])
    zs, xts = inv[0]
    outs = []
    try:
        for share in (True, False):
            cb = _batch_controller(hip, pairs, T, K)
            edit, recon = HEditEngine(hip, share_latents=share).run(
                xts[T].contiguous(), zs, prompt_pairs, [1.0, 5.0, 7.5], cb, eta=1.0, p2p=True, implicit=True, K=K, w_rec=0.1,
                after_skip_steps=T, ddim_inv=False, fuse_src_pass=fuse)
            G.sync()
            maps = [m.clone() for key in sorted(cb.attention_store) for m in cb.attention_store[key]]
            outs.append((edit, recon, maps))
    finally:
        _unregister(hip)
    return outs, xts


def _assert_same_loop(outs):
    (e1, r1, m1), (e0, r0, m0) = outs
    assert torch.isfinite(e1).all()
    assert torch.equal(e1, e0) and torch.equal(r1, r0)
    assert len(m1) == len(m0) and len(m1) > 0
    for a, b in zip(m1, m0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fuse", [True, False], ids=["fuse_src_pass", "separate_src_pass"])
def test_p2p_loop_at_4096_tokens_shares_under_the_plan(tiny4, fuse):
    """64 x 64 latents: the first block is outside the self-replace window's reach and stores nothing, so the 4n / 5n-row P2P passes
    share too (the non-chain transformer path); edit, reconstruction and the stored cross maps keep their bits"""
    outs, xts = _loop_both_ways(tiny4, 64, 3, 4, 2, fuse, 21)
    _assert_same_loop(outs)
    assert torch.equal(outs[0][1], xts[0])


def test_p2p_loop_at_1024_tokens_falls_back_inside_the_self_window(tiny):
    """32 x 32 latents: inside the self-replace window qk_src reaches the first block, those calls spread the latents to one per
    row and take the plain path; the others share"""
    outs, xts = _loop_both_ways(tiny, 32, 3, 4, 2, True, 31)
    _assert_same_loop(outs)
    assert torch.equal(outs[0][1], xts[0])


def test_hooked_call_next_to_a_shared_call(tiny):
    """the hook path (workspace sized with the hook set, never shared) and a shared call on one handle, either order"""
    unet = tiny.unet
    rmap = [0, 1, 0, 1]
    x, ctx = _inputs(2, 4, TINY_CONFIG, 32, 9)
    rows = x[rmap].contiguous()
    want = unet.forward_raw(rows, 401.0, ctx)
    seen = []

    def watch(attn, is_cross, place, save_attn):
        seen.append((tuple(attn.shape), is_cross))

    _shared_vs_rows(unet, x, ctx, rmap, 401.0)
    hooked = unet.forward_hooked(rows, 401.0, ctx, watch)
    G.sync()
    assert len(seen) > 0 and torch.isfinite(hooked).all()
    _shared_vs_rows(unet, x, ctx, rmap, 401.0)
    assert torch.equal(unet.forward_raw(rows, 401.0, ctx), want)


SD15_MAPS = [[0, 1, 0, 1, 1], [0, 1, 0, 1]]


@pytest.mark.parametrize("rmap", SD15_MAPS, ids=["5-rows", "4-rows"])
def test_sd15_chain_path_without_a_plan(sd15, rmap):
    x, ctx = _inputs(2, len(rmap), SD15_CONFIG, 64, 3 + len(rmap))
    _shared_vs_rows(sd15.unet, x, ctx, rmap, 481.0)


@pytest.mark.parametrize("rmap", SD15_MAPS, ids=["5-rows", "4-rows"])
@pytest.mark.parametrize("step", [0, 6], ids=["inside-self-window", "after-self-window"])
def test_sd15_chain_path_under_the_batch_controllers_plan(sd15, rmap, step):
    """one image, rows [x_orig|null, x_k|null, x_orig|src, x_k|tar (, x_k|src)]: the plan of a 10-step schedule at step 0 (self-replace
    on: window [0, 3)) and at step 6 (off); at 4096 tokens neither reaches the first block"""
    T = 10
    x, ctx = _inputs(2, len(rmap), SD15_CONFIG, 64, 13 + len(rmap))
    try:
        cb = _batch_controller(sd15, [PROMPT_PAIRS[0]], T, 1)
        assert cb._self_window()[0] <= 0 < cb._self_window()[1] <= 6
        cb.cur_step = step
        plan = cb._plan(sd15.unet, len(rmap), 64, 64, True)
        assert bool(plan.qk_src) == (step == 0)
        _shared_vs_rows(sd15.unet, x, ctx, rmap, 481.0, plan)
    finally:
        _unregister(sd15)


def test_sd15_reconstruction_still_retraces_the_inversion(sd15):
    """3 steps, 2 images, P2P + LocalBlend, the 5n-row pass: inversion ([xt, xt] shared) and loop (base and P2P passes shared)"""
    try:
        outs, xts = _loop_both_ways(sd15, 64, 2, 3, 1, True, 7)
    finally:
        sd15.scheduler.set_timesteps(10)
    _assert_same_loop(outs)
    assert torch.equal(outs[0][1], xts[0])
