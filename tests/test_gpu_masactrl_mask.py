"""-m gpu: mask-guided MasaCtrl on the HIP path -- the class-matched self-attention kernel (csrc/maskattn.hip) through the C
ABI, the executor's split into source rows (plain kernel, today's bits) and target rows (class-matched kernel), and the
``MutualSelfAttentionControlMask`` editor in the h-Edit loop and the lock-step engine."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import gpu as G  # noqa: E402
from helpers.models import make_pair  # noqa: E402
from helpers.tiny import PROMPT_PAIRS  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.unet import TINY_CONFIG  # noqa: E402

T = 8
SHAPES = [(2, 32, 64), (4, 64, 256), (8, 40, 1024), (8, 80, 256), (8, 160, 64)]
KV = [0, 0, 2, 2]


def operands(B, heads, d, N, seed):
    Cc = heads * d
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, N, Cc, generator=g) * 0.5 for _ in range(3))
    scale = d ** -0.5 * 1.4426950408889634
    qk = torch.cat([q * scale, k], dim=-1).to(_lib.storage_dtype()).to(G.dev()).contiguous()
    vt = v.to(_lib.storage_dtype()).permute(2, 0, 1).reshape(Cc, B * N).contiguous().to(G.dev())
    st = lambda t: t.to(_lib.storage_dtype()).double().reshape(B, N, heads, d).transpose(1, 2)   # storage-rounded, (B, h, N, d)
    return qk, vt, st(q), st(k), st(v)


def launch(qk, vt, out, B, N, heads, d, rows, kv, cls_q, cls_k):
    Cc = heads * d
    lib = _lib.lib()
    rows_t = torch.tensor(rows, dtype=torch.int32, device=G.dev())
    kv_t = torch.tensor(kv, dtype=torch.int32, device=G.dev())
    k_view = qk.view(-1, qk.shape[-1])[:, qk.shape[-1] // 2:]
    _lib.check(lib.hedit_k_masked_self_attn(_lib.ptr(qk), 2 * Cc, C.c_void_p(k_view.data_ptr()), 2 * Cc, _lib.ptr(vt), B * N,
                                            _lib.ptr(out), Cc, B, N, heads, d, _lib.ptr(rows_t), len(rows), _lib.ptr(kv_t),
                                            _lib.ptr(cls_q), _lib.ptr(cls_k), None))
    G.sync()


def reference(qd, kd, vd, d, b, kb, cq, ck):
    """fp64, one softmax per query over the keys of its class; a class without keys: the mean of V"""
    s = qd[b] @ kd[kb].transpose(-1, -2) * d ** -0.5                      # (h, N, N)
    adm = cq[b].bool()[:, None] == ck[kb].bool()[None, :]                 # (N, N)
    empty = ~adm.any(dim=1)
    s = s.masked_fill(~adm[None], float("-inf"))
    s[:, empty, :] = 0.0
    return torch.softmax(s, -1) @ vd[kb]                                  # (h, N, d)


def masks(kind, B, N, seed):
    """(cls_q, cls_k) uint8 [B][N]; query classes matter on rows 1, 3, key classes on rows 0, 2"""
    g = torch.Generator().manual_seed(seed)
    r = int(N ** 0.5)
    if kind == "bernoulli":
        cq = (torch.rand(B, N, generator=g) < 0.5)
        ck = (torch.rand(B, N, generator=g) < 0.5)
    elif kind == "halves":            # keys: upper half of the image; queries: left half -> pure key tiles under mixed query blocks (nothing skipped)
        yy, xx = torch.meshgrid(torch.arange(r), torch.arange(r), indexing="ij")
        ck = (yy < r // 2).reshape(1, N).expand(B, N)
        cq = (xx < r // 2).reshape(1, N).expand(B, N)
    elif kind == "planes":            # keys AND queries: upper half of the image.  A block of 128 queries is then pure
        # (N >= 256: the first N / 2 queries are whole blocks), and so is every 64-key tile: the upper blocks want class 1
        # only and skip the all-0 tiles, the lower blocks want class 0 only and skip the all-1 tiles -- the tile-skip branch
        ck = (torch.arange(N) < N // 2).reshape(1, N).expand(B, N)
        cq = ck
    elif kind == "planes_swapped":    # the same tiles against the other class: queries of the LOWER half are foreground
        ck = (torch.arange(N) < N // 2).reshape(1, N).expand(B, N)
        cq = ~ck
    elif kind == "empty":             # source all foreground, mixed target: background queries have no key
        ck = torch.ones(B, N, dtype=torch.bool)
        cq = (torch.rand(B, N, generator=g) < 0.5)
    elif kind == "single":            # exactly one foreground key
        ck = torch.zeros(B, N, dtype=torch.bool)
        ck[:, N // 3] = True
        cq = (torch.rand(B, N, generator=g) < 0.5)
    elif kind == "ones":
        cq = torch.ones(B, N, dtype=torch.bool)
        ck = torch.ones(B, N, dtype=torch.bool)
    return cq.to(torch.uint8).contiguous(), ck.to(torch.uint8).contiguous()


@pytest.mark.parametrize("kind", ["bernoulli", "halves", "empty", "single"])
@pytest.mark.parametrize("heads,d,N", SHAPES)
def test_kernel_matches_fp64(heads, d, N, kind):
    B, Cc, rows = 4, heads * d, [1, 3]
    qk, vt, qd, kd, vd = operands(B, heads, d, N, heads * 1000 + N)
    cq, ck = masks(kind, B, N, N + d)
    sentinel = torch.full((B, N, Cc), 7.0, dtype=_lib.storage_dtype(), device=G.dev())
    out = sentinel.clone()
    launch(qk, vt, out, B, N, heads, d, rows, KV, cq.to(G.dev()), ck.to(G.dev()))
    for b in (0, 2):
        assert torch.equal(out[b].view(torch.int16), sentinel[b].view(torch.int16)), "an unlisted row was written"
    for b in rows:
        want = reference(qd, kd, vd, d, b, KV[b], cq, ck)                 # (h, N, d)
        got = out[b].double().cpu().reshape(N, heads, d).transpose(0, 1)
        G.within(G.rel_err(got, want), 1.2e-2, what=f"{kind} row {b}")
        if kind == "empty":
            sel = cq[b] == 0                                              # no background key: the mean of V
            mean_v = vd[KV[b]].mean(dim=1, keepdim=True).expand(-1, int(sel.sum()), -1)
            G.within(G.rel_err(got[:, sel], mean_v), 1.2e-2, what="empty class -> mean of V")
        if kind == "single":
            sel = cq[b] == 1                                              # one foreground key: its V row
            one_v = vd[KV[b]][:, N // 3][:, None].expand(-1, int(sel.sum()), -1)
            G.within(G.rel_err(got[:, sel], one_v), 1.2e-2, what="single key -> its V row")


@pytest.mark.parametrize("kind", ["planes", "planes_swapped"])
@pytest.mark.parametrize("heads,d,N", [(4, 64, 256), (8, 40, 1024), (8, 80, 256), (2, 32, 384)])
def test_kernel_skips_only_tiles_nobody_wants(heads, d, N, kind):
    """query blocks of ONE class against key tiles of one class: want = class 0 only against all-1 tiles and want = class 1
    only against all-0 tiles, both skipped, against the same fp64 reference.  (The other mask kinds never reach the skip: their
    128-query blocks hold both classes.)  N = 384: the class boundary at query 192 cuts a block, so block 1 is mixed and must
    load every tile while blocks 0 and 2 skip half of them."""
    B, Cc, rows = 4, heads * d, [1, 3]
    qk, vt, qd, kd, vd = operands(B, heads, d, N, heads * 1000 + N + 7)
    cq, ck = masks(kind, B, N, 0)
    for blk in range(0, N, 128):                           # the property the test is about, stated on its inputs
        pure = len(set(cq[1, blk:blk + 128].tolist())) == 1
        assert pure == (N != 384 or blk != 128)
    assert all(len(set(ck[0, t:t + 64].tolist())) == 1 for t in range(0, N, 64))
    out = torch.full((B, N, Cc), 7.0, dtype=_lib.storage_dtype(), device=G.dev())
    launch(qk, vt, out, B, N, heads, d, rows, KV, cq.contiguous().to(G.dev()), ck.contiguous().to(G.dev()))
    for b in rows:
        want = reference(qd, kd, vd, d, b, KV[b], cq, ck)
        got = out[b].double().cpu().reshape(N, heads, d).transpose(0, 1)
        G.within(G.rel_err(got, want), 1.2e-2, what=f"{kind} row {b}")
        for half in (slice(0, N // 2), slice(N // 2, N)):  # each class on its own: an error in one is not averaged away
            G.within(G.rel_err(got[:, half], want[:, half]), 1.2e-2, what=f"{kind} row {b} half")


@pytest.mark.parametrize("heads,d,N", SHAPES)
def test_all_ones_masks_agree_with_mutual_attention(heads, d, N):
    B, Cc, rows = 4, heads * d, [1, 3]
    qk, vt, _, _, _ = operands(B, heads, d, N, heads * 1000 + N + 1)
    cq, ck = masks("ones", B, N, 0)
    out = torch.zeros(B, N, Cc, dtype=_lib.storage_dtype(), device=G.dev())
    launch(qk, vt, out, B, N, heads, d, rows, KV, cq.to(G.dev()), ck.to(G.dev()))
    plain = torch.empty_like(out)
    kv_t = torch.tensor(KV, dtype=torch.int32, device=G.dev())
    k_view = qk.view(B * N, 2 * Cc)[:, Cc:]
    _lib.check(_lib.lib().hedit_k_self_attn(_lib.ptr(qk), 2 * Cc, C.c_void_p(k_view.data_ptr()), 2 * Cc, _lib.ptr(vt), B * N,
                                            _lib.ptr(plain), Cc, B, N, heads, d, None, _lib.ptr(kv_t), None))
    G.sync()
    G.within(G.rel_err(out[rows].float(), plain[rows].float()), 1.2e-2)


@pytest.mark.parametrize("heads,d,N", [(8, 40, 256), (8, 160, 64), (4, 64, 192)])
def test_rows_have_the_same_bits_in_any_batch(heads, d, N):
    """B = 8 with rows [2, 3, 6, 7] against two B = 4 launches on the halves; and the list reversed"""
    B, Cc = 8, heads * d
    qk, vt, _, _, _ = operands(B, heads, d, N, 77 + N)
    cq, ck = masks("bernoulli", B, N, 5)
    cq[3] = 1                                      # one row with an empty class in it
    ck[1] = 0
    kv = [0, 1, 0, 1, 4, 5, 4, 5]
    cqd, ckd = cq.to(G.dev()), ck.to(G.dev())
    bits = lambda t: t.view(torch.int16)
    full = torch.zeros(B, N, Cc, dtype=_lib.storage_dtype(), device=G.dev())
    launch(qk, vt, full, B, N, heads, d, [2, 3, 6, 7], kv, cqd, ckd)
    rev = torch.zeros_like(full)
    launch(qk, vt, rev, B, N, heads, d, [7, 6, 3, 2], kv, cqd, ckd)
    assert torch.equal(bits(full), bits(rev))
    vt3 = vt.view(Cc, B, N)
    for half in (0, 1):
        sl = slice(4 * half, 4 * half + 4)
        out = torch.zeros(4, N, Cc, dtype=_lib.storage_dtype(), device=G.dev())
        launch(qk[sl].contiguous(), vt3[:, sl].reshape(Cc, 4 * N).contiguous(), out, 4, N, heads, d, [2, 3], [0, 1, 0, 1],
               cqd[sl].contiguous(), ckd[sl].contiguous())
        assert torch.equal(bits(out[2:]), bits(full[sl][2:]))


def test_shapes_outside_the_kernel_are_refused_by_name():
    qk, vt, _, _, _ = operands(4, 2, 32, 64, 1)
    cq, ck = masks("ones", 4, 64, 0)
    out = torch.zeros(4, 64, 64, dtype=_lib.storage_dtype(), device=G.dev())
    with pytest.raises(_lib.HipError, match="multiple of 64"):
        launch(qk, vt, out, 4, 32, 2, 32, [1, 3], KV, cq.to(G.dev()), ck.to(G.dev()))
    with pytest.raises(_lib.HipError, match="head dim"):
        launch(qk, vt, out, 4, 64, 4, 16, [1, 3], KV, cq.to(G.dev()), ck.to(G.dev()))


# ------------------------------------------------------------------------------------------ executor, loop, engine
@pytest.fixture(scope="module")
def setup():
    from oracle import loops as OL
    hip, om, _ = make_pair(TINY_CONFIG, T, out_scale=0.3)
    torch.manual_seed(11)
    w0 = torch.randn(1, 4, 32, 32) * 0.8
    torch.manual_seed(100)
    zs, wts, _ = OL.ddpm_inversion(om, w0, eta=1.0, prompt=PROMPT_PAIRS[0][0], cfg_src=1.0, T=T)
    return hip, om, zs, wts


def square(h=32, lo=8, hi=24):
    m = torch.zeros(h, h)
    m[lo:hi, lo:hi] = 1
    return m


def run_loop(hip, zs, wts, editor, skip=4, K=1):
    from hedit.inversion.masactrl_h_edit import h_Edit_masactrl_implicit
    from hedit.masactrl import regiter_attention_editor_diffusers
    regiter_attention_editor_diffusers(hip, editor)
    after = T - skip
    e, r = h_Edit_masactrl_implicit(hip, xT=G.f32(wts[after]), zs=G.f32(zs[:after]), prog_bar=False, eta=1.0,
                                    prompts=[PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]], cfg_scales=[1.0, 5.0, 7.5],
                                    optimization_steps=K, after_skip_steps=after, is_ddim_inversion=False)
    G.sync()
    return e, r


def test_source_rows_never_see_a_mask(setup):
    """reconstruction bit-equal to the plain editor's, the edit moved by the masks; all-ones masks: the plain edit again"""
    from hedit.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    hip, _, zs, wts = setup
    e_p, r_p = run_loop(hip, zs, wts, MutualSelfAttentionControl(0, 0))
    e_m, r_m = run_loop(hip, zs, wts, MutualSelfAttentionControlMask(0, 0, mask_s=square(), mask_t=square()))
    assert torch.isfinite(e_m).all()
    assert torch.equal(r_m, r_p)
    assert G.rel_err(e_m, e_p) > 1e-2
    ones = torch.ones(32, 32)
    e_1, r_1 = run_loop(hip, zs, wts, MutualSelfAttentionControlMask(0, 0, mask_s=ones, mask_t=ones))
    assert torch.equal(r_1, r_p)
    G.within(G.rel_err(e_1, e_p), 8e-2)


def test_engine_batch_is_bit_equal_per_image(setup):
    """n = 2 with (2, h, w) masks against the two n = 1 runs"""
    from hedit.engine import HEditEngine
    from hedit.masactrl import MutualSelfAttentionControlMask, regiter_attention_editor_diffusers
    hip, _, zs, wts = setup
    after = 4
    m = torch.stack([square(), square(32, 4, 14)])
    pairs = [[PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]], [PROMPT_PAIRS[1][0], PROMPT_PAIRS[1][1]]]
    torch.manual_seed(5)
    x = G.f32(torch.stack([wts[after], wts[after] + 0.1 * torch.randn(4, 32, 32)]))       # (2, 4, 32, 32)
    z = G.f32(torch.stack([zs[:after], zs[:after].flip(-1)], dim=1))                        # (T', 2, 4, 32, 32)

    def run(sel):
        ed = MutualSelfAttentionControlMask(0, 0, mask_s=m[sel], mask_t=m[sel])
        regiter_attention_editor_diffusers(hip, ed)
        e, r = HEditEngine(hip).run(x[sel].contiguous(), z[:, sel].contiguous(), [pairs[i] for i in sel], [1.0, 5.0, 7.5], ed, eta=1.0,
                                    p2p=True, implicit=True, K=1, after_skip_steps=after, ddim_inv=False, rec_pull=False)
        G.sync()
        return e, r

    e2, r2 = run([0, 1])
    for i in (0, 1):
        e1, r1 = run([i])
        assert torch.equal(e2[i:i + 1], e1) and torch.equal(r2[i:i + 1], r1)


def test_executor_refuses_what_it_cannot_run_by_name(setup):
    """before anything is launched: classes under the host-language hook, without kv_src, on a non-square latent"""
    from hedit.masactrl import MutualSelfAttentionControlMask
    hip, _, _, _ = setup
    unet = hip.unet
    ed = MutualSelfAttentionControlMask(0, 0, mask_s=square(), mask_t=square())
    x = torch.zeros(4, 4, 32, 32, device=G.dev())
    ctx = torch.zeros(4, 77, TINY_CONFIG["cross_attention_dim"], device=G.dev())
    p = ed._plan(unet, 4, 32, 32, True)
    assert p.n_masa_rows == 2
    unet.forward_raw(x, 1.0, ctx, p)                                          # the plan as compiled runs
    kv, p.kv_src = p.kv_src, None
    with pytest.raises(_lib.HipError, match="masa classes need kv_src"):
        unet.forward_raw(x, 1.0, ctx, p)
    p.kv_src = kv
    with pytest.raises(_lib.HipError, match="non-square"):
        unet.forward_raw(torch.zeros(4, 4, 32, 64, device=G.dev()), 1.0, ctx, p)
    fn = unet._HOOK_T(lambda *a: 0)
    _lib.check(unet._lib.hedit_unet_set_attn_hook(unet._h, C.cast(fn, C.c_void_p), None))
    try:
        with pytest.raises(_lib.HipError, match="attention hook cannot run class-matched"):
            unet.forward_raw(x, 1.0, ctx, p)
    finally:
        _lib.check(unet._lib.hedit_unet_set_attn_hook(unet._h, None, None))
    G.sync()


@pytest.mark.parametrize("skip,K,step,layer", [(4, 1, 1, 2), (4, 2, 0, 0)])
def test_masked_loop_matches_the_oracle(setup, skip, K, step, layer):
    """given masks (a centred square) against the oracle UNet with the fp64 restatement of the reference's editor; the
    project's limits for these cases (tests/test_gpu_masactrl.py)"""
    from oracle import loops as OL
    from helpers import masactrl_mask_ref as MR
    from hedit.masactrl import MutualSelfAttentionControlMask
    hip, om, zs, wts = setup
    after = T - skip
    ed_o = MR.MaskEditor(step, layer, mode="given", mask_s=square(), mask_t=square())
    MR.register_editor(om, ed_o)
    e_o, r_o = OL.h_edit_masactrl_implicit(om, wts[after], zs=zs[:after], eta=1.0, prompts=[PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]],
                                           cfg_scales=[1.0, 5.0, 7.5], optimization_steps=K, after_skip_steps=after,
                                           is_ddim_inversion=False)
    ed_h = MutualSelfAttentionControlMask(step, layer, mask_s=square(), mask_t=square())
    e_h, r_h = run_loop(hip, zs, wts, ed_h, skip, K)
    assert ed_h.cur_step == ed_o.cur_step == after * K
    err_r, err_e = G.rel_err(r_h, r_o), G.rel_err(e_h, e_o)
    print(f"masked loop skip={skip} K={K} step={step} layer={layer}: recon {err_r:.3e} edit {err_e:.3e}")
    G.within(err_r, 1e-2)
    G.within(err_e, 8e-2)


# ------------------------------------------------------------------------------------------ auto variant
@pytest.mark.parametrize("rows,heads", [(2, 2), (4, 8), (2, 8), (4, 2)])
def test_accumulate_matches_fp64(rows, heads):
    g = torch.Generator().manual_seed(rows * 10 + heads)
    probs = torch.softmax(2.0 * torch.randn(rows * heads, 256, 77, generator=g), dim=-1)
    acc0 = torch.rand(rows, 256, generator=g)
    ref, cur = [1, 3, 76], [2]
    acc = acc0.clone().to(G.dev())
    ref_t, cur_t = (torch.tensor(v, dtype=torch.int32, device=G.dev()) for v in (ref, cur))
    _lib.check(_lib.lib().hedit_k_masa_accumulate(_lib.ptr(G.f32(probs)), heads, rows, _lib.ptr(ref_t), len(ref), _lib.ptr(cur_t), len(cur),
                                                  _lib.ptr(acc), None))
    G.sync()
    p = probs.double().reshape(rows, heads, 256, 77).mean(1)                 # (rows, 256, 77)
    want = acc0.double() + torch.cat([p[:rows // 2][..., ref].sum(-1), p[rows // 2:][..., cur].sum(-1)])
    assert G.rel_err(acc, want) < 1e-5
    assert ((acc.double().cpu() - want).abs() / want.abs()).max().item() < 1e-5


def grid_maps(seed, n, avoid):
    """[2 n][256] maps with values k / 32, min 0 and max 1 present, no value within 1e-4 of `avoid`"""
    g = torch.Generator().manual_seed(seed)
    ks = [k for k in range(33) if abs(k / 32 - avoid) > 1e-3]
    m = torch.tensor(ks, dtype=torch.float32)[torch.randint(0, len(ks), (2 * n, 256), generator=g)] / 32
    m[:, 7], m[:, 200] = 0.0, 1.0
    return m


@pytest.mark.parametrize("thres", [0.1, 0.5])
@pytest.mark.parametrize("res", [8, 16, 32, 64])
def test_auto_mask_matches_the_helper(res, thres):
    from helpers import masactrl_mask_ref as MR
    n, count, N = 2, 3, res * res
    maps = grid_maps(res, n, thres)
    # shifted and scaled so that the normalisation has work to do; the accumulator holds the SUM over `count` layers
    raw = 0.25 + 0.5 * maps
    acc = (raw * count).to(G.dev())
    cls = torch.full((4 * n, N), 9, dtype=torch.uint8, device=G.dev())
    _lib.check(_lib.lib().hedit_k_masa_auto_mask(_lib.ptr(acc), count, n, res, C.c_float(thres), _lib.ptr(cls), None))
    G.sync()
    cls = cls.cpu()
    for i in range(n):
        cross = torch.zeros(4, 256, 77, dtype=torch.float64)
        cross[2, :, 5] = raw[i].double()                                      # the conditional source row's map, token 5
        cross[3, :, 6] = raw[n + i].double()                                  # the conditional target row's map, token 6
        ms, mt, ns, nt = MR.auto_masks([cross], [5], [6], thres, res)
        assert ((ns - thres).abs() > 1e-4).all() and ((nt - thres).abs() > 1e-4).all()      # a condition on the inputs
        assert 0 < ms.sum() < N and 0 < mt.sum() < N
        for row, want in ((i, ms), (2 * n + i, ms), (n + i, mt), (3 * n + i, mt)):
            assert torch.equal(cls[row], want.to(torch.uint8)), (row, res, thres)


def test_auto_mask_of_a_constant_map_is_background():
    n, res = 1, 16
    acc = torch.full((2, 256), 0.37, device=G.dev())
    cls = torch.full((4, res * res), 9, dtype=torch.uint8, device=G.dev())
    _lib.check(_lib.lib().hedit_k_masa_auto_mask(_lib.ptr(acc), 2, n, res, C.c_float(0.1), _lib.ptr(cls), None))
    G.sync()
    assert int(cls.sum()) == 0


def auto_run(hip, zs, wts, start_layer, **kw):
    from hedit.masactrl import MutualSelfAttentionControlMaskAuto
    ed = MutualSelfAttentionControlMaskAuto(1, start_layer, thres=0.3, ref_token_idx=[3], cur_token_idx=[3], keep_masks=True, **kw)
    e, r = run_loop(hip, zs, wts, ed)
    return ed, e, r


def test_auto_loop_matches_the_oracle_on_the_devices_masks(setup, tmp_path):
    """The masks come from bf16 attention and are thresholded, so the oracle replays the masks the device formed (a pixel
    at the threshold would flip between the two otherwise); everything downstream of the masks is compared."""
    from oracle import loops as OL
    from helpers import masactrl_mask_ref as MR
    hip, om, zs, wts = setup
    ed_h, e_h, r_h = auto_run(hip, zs, wts, 4, mask_save_dir=str(tmp_path))
    active = {(s, b) for s in (1, 2, 3) for b in range(4, 11)}                # 4 steps; the tiny UNet has 11 blocks
    assert set(ed_h.saved_masks) == active
    res = {4: 8, 5: 16, 6: 16, 7: 16, 8: 32, 9: 32, 10: 32}
    for (s, b), (src, tar) in ed_h.saved_masks.items():
        assert src.shape == tar.shape == (1, res[b], res[b]) and int(src.max()) <= 1
        assert 0 < int(src.sum()) < src.numel() and 0 < int(tar.sum()) < tar.numel(), "a constant mask"
    assert sorted(os.listdir(tmp_path))[:2] == ["mask_s_1_10.png", "mask_s_1_12.png"] and len(os.listdir(tmp_path)) == 2 * len(active)
    ed_o = MR.MaskEditor(1, 4, mode="replay", masks={key: (m[0][0], m[1][0]) for key, m in ed_h.saved_masks.items()})
    MR.register_editor(om, ed_o)
    e_o, r_o = OL.h_edit_masactrl_implicit(om, wts[4], zs=zs[:4], eta=1.0, prompts=[PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]],
                                           cfg_scales=[1.0, 5.0, 7.5], optimization_steps=1, after_skip_steps=4, is_ddim_inversion=False)
    assert set(ed_o.used) == active
    err_r, err_e = G.rel_err(r_h, r_o), G.rel_err(e_h, e_o)
    print(f"auto loop: recon {err_r:.3e} edit {err_e:.3e}")
    G.within(err_r, 1e-2)
    G.within(err_e, 8e-2)
    # the share of pixels where the device's masks differ from the oracle's own (fp32 maps): reported, not asserted
    ed_a = MR.MaskEditor(1, 4, mode="auto", thres=0.3, ref_idx=(3,), cur_idx=(3,))
    MR.register_editor(om, ed_a)
    OL.h_edit_masactrl_implicit(om, wts[4], zs=zs[:4], eta=1.0, prompts=[PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]],
                                cfg_scales=[1.0, 5.0, 7.5], optimization_steps=1, after_skip_steps=4, is_ddim_inversion=False)
    diff = tot = 0
    for key, (src, tar) in ed_h.saved_masks.items():
        ms, mt = ed_a.used[key]
        diff += int((src.reshape(-1) != ms.to(torch.uint8)).sum()) + int((tar.reshape(-1) != mt.to(torch.uint8)).sum())
        tot += 2 * src.numel()
    print(f"auto loop: {diff} of {tot} mask pixels differ from the fp64 oracle's own masks ({100.0 * diff / tot:.2f} %)")


def test_auto_layers_without_a_map_run_unmasked(setup):
    hip, _, zs, wts = setup
    ed0, e0, r0 = auto_run(hip, zs, wts, 0)
    # blocks 0 .. 2 come before the first 256-token cross-attention has been folded in (block 2's own follows its self layer)
    assert {b for (_, b) in ed0.saved_masks} == set(range(3, 11)) and {s for (s, _) in ed0.saved_masks} == {1, 2, 3}
    ed4, e4, r4 = auto_run(hip, zs, wts, 4)
    assert torch.equal(r0, r4)                                                # source rows: untouched either way
    assert G.rel_err(e0, e4) > 1e-3


def test_driver_masa_mask_pie_batch_writes_the_same_bytes(tmp_path):
    """main_masactrl.py --masa_mask pie: --batch 2 writes --batch 1's bytes (h-Edit-D draws no random numbers), into a directory
    named ..._mask_pie, and the images differ from the run without masks"""
    import importlib.util
    import numpy as np
    from PIL import Image
    from helpers.datasets import pie_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hedit_main_masactrl_pie", os.path.join(root, "h-edit_amd", "main_masactrl.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    d = pie_dataset(tmp_path)
    import json
    with open(d / "mapping_file.json") as f:
        mapping = json.load(f)
    for i, item in enumerate(mapping.values()):             # run-length edit masks: a block of rows, another per entry
        item["mask"] = [512 * (96 + 64 * i), 512 * 200]
    with open(d / "mapping_file.json", "w") as f:
        json.dump(mapping, f)
    common = ["--data_path", str(d), "--random_init", "--tiny", "--num_diffusion_steps", "4", "--edit_category_list", "0", "7",
              "--step", "1", "--layer", "2"]
    none = drv.main(common + ["--output_path", str(tmp_path / "r0")])
    one = drv.main(common + ["--output_path", str(tmp_path / "r1"), "--masa_mask", "pie"])
    two = drv.main(common + ["--output_path", str(tmp_path / "r2"), "--masa_mask", "pie", "--batch", "2"])
    assert len(none) == len(one) == len(two) == 2
    differ = 0
    for a, b, c in zip(sorted(none), sorted(one), sorted(two)):
        sub_a, sub_b = os.path.relpath(a, tmp_path / "r0"), os.path.relpath(b, tmp_path / "r1")      # (the test's own name is in tmp_path)
        assert "_step_1_layer_2__mask_pie" + os.sep in sub_b and "_mask_pie" not in sub_a and "_step_1_layer_2_" + os.sep in sub_a
        assert os.path.basename(b) == os.path.basename(c)
        assert np.array_equal(np.array(Image.open(b)), np.array(Image.open(c)))
        differ += int(not np.array_equal(np.array(Image.open(a)), np.array(Image.open(b))))
    assert differ > 0


@pytest.mark.parametrize("which", ["Mask", "MaskAuto"])
def test_gradient_pass_refuses_the_mask_editors_by_name(which):
    """the input-gradient pass differentiates the plain network only: a registered mask-guided editor is refused with its name"""
    from hedit.masactrl import MutualSelfAttentionControlMask, MutualSelfAttentionControlMaskAuto
    from hedit.unet import UNet2DConditionModel
    unet = UNet2DConditionModel(TINY_CONFIG, device="cuda:0", grad=True)
    unet.init_random(0)
    ed = (MutualSelfAttentionControlMask(0, 0, mask_s=square(), mask_t=square()) if which == "Mask"
          else MutualSelfAttentionControlMaskAuto(0, 0))
    unet._attention_editor = ed
    x = torch.zeros(4, 4, 32, 32, device=G.dev(), requires_grad=True)
    ctx = torch.zeros(4, 77, TINY_CONFIG["cross_attention_dim"], device=G.dev())
    with pytest.raises(NotImplementedError, match=f"MutualSelfAttentionControl{which}\\) is in the way"):
        unet(x, 401.0, encoder_hidden_states=ctx)
    assert unet(x, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs={"use_editor": False}).sample.requires_grad
    G.sync()
