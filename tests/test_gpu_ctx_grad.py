"""-m gpu: the gradient with respect to the TEXT CONTEXT -- the cross-attention dk / dv kernels (csrc/attnbwd.hip, the context
form: split over the queries, fixed-order reduction) through the C ABI against fp64 torch.autograd; the executor built on them
(csrc/unetgrad.h: hedit_unet_backward_ctx on a handle from hedit_unet_create_grad_ctx) and its autograd facade
(hedit.unet.UNet2DConditionModel(grad="context")) against torch.autograd on the fp32 CPU oracle (oracle/sd_unet.py); one
null-text update of hedit.inversion.pnp_baselines.nulltext_pnp, and the main_nt.py driver.

Tolerances (relative L2, through G.within: half storage gets a quarter):

* dk, dv of the kernel, 6e-3: the attention-backward limit of tests/test_gpu_unet_grad.py -- the same roundings (P and dS to
  storage before their products), and the reduction over the queries is the one that file's dk / dv have; the only addition is
  that the fp32 chain is cut into chunks of 128 queries whose fp32 partials are added in fp32.
* d_ctx of the executor: measured on the CPU as tests/test_gpu_unet_grad.py did for d_x (bf16 autocast of the oracle against
  the oracle itself, TINY_CONFIG, 32 x 32, the inputs of test_d_ctx_matches_oracle_autograd: B = 2, t = 501, seed 30): d_x moves
  by 2.35e-2 (that file's 2.5e-2), d_ctx by 2.70e-2 (2.67e-2 at t = 21, 2.84e-2 for one image at t = 301).  That is above
  2.5e-2, so the limit is 1.6 times the measured value: 1.6 x 2.704e-2 = 4.33e-2.

What moves bits only (batch rows, repeated calls, d_x = NULL, the facade) is compared with torch.equal."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers.tiny import hash_normal  # noqa: E402
from hedit import _lib  # noqa: E402
from test_gpu_unet_grad import CTX, CTXP, ERR_ARG, ERR_STATE, Net, attn_case, dt  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 128                    # queries per block of the partial kernel (csrc/attnbwd.hip: CTX_CHUNK)
TOL_DCTX = 1.6 * 2.704e-2      # module docstring
# hedit_unet_grad_workspace_bytes(h, 1, 32, 32) of a hedit_unet_create_grad handle on TINY_CONFIG, recorded on the commit before
# the context gradient existed: that handle's plan must not have moved
WS_TINY_1_32 = 23995392


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


# ---------------------------------------------------------------------------------------------- the kernel
def run_kv(lib, c, B, heads, N, d, rows=None):
    """hedit_k_cross_attn_bwd_kv on the images `rows` of a case.  Pad rows of k and v are NaN (never read), dk / dv are
    pre-filled with NaN (every element written) -> ([Bn][80][C], [Bn][80][C])"""
    C_ = heads * d
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    q, k, v, o, do = (sel(c[n]) for n in ("q", "k", "v", "o", "do"))
    Bn = q.shape[0]

    def padded(t):
        out = torch.full((Bn, CTXP, C_), float("nan"))
        out[:, :CTX] = t
        return G.bf(out.reshape(Bn * CTXP, C_))

    kd, vd = padded(k), padded(v)
    qd, od, dod = (G.bf(t.reshape(Bn * N, C_)) for t in (q, o, do))
    dk, dv = (torch.full((Bn * CTXP, C_), float("nan"), dtype=dt(), device=G.dev()) for _ in range(2))
    need = lib.hedit_k_cross_attn_bwd_kv_ws_bytes(Bn, N, heads, d)
    chunks = (N + CHUNK - 1) // CHUNK
    assert need == Bn * heads * N * 8 + 2 * Bn * heads * chunks * CTXP * d * 4
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=G.dev())
    _lib.check(lib.hedit_k_cross_attn_bwd_kv(_lib.ptr(qd), C_, _lib.ptr(kd), C_, _lib.ptr(vd), C_, _lib.ptr(od), C_, _lib.ptr(dod), C_,
                                             _lib.ptr(dk), _lib.ptr(dv), C_, Bn, N, heads, d, _lib.ptr(ws), None))
    G.sync()
    return dk.reshape(Bn, CTXP, C_), dv.reshape(Bn, CTXP, C_)


# (B, heads, N, d): one tile row of queries; pad 40 -> 48 with head and batch offsets, one full chunk; d = 160 (the largest LDS
# image); an odd tile count in two chunks with batch offsets; one chunk + 64 (two chunks, the last shorter); SD's 32 x 32 level
KV_SHAPES = [(1, 2, 64, 32), (2, 2, 128, 40), (1, 1, 64, 160), (2, 1, 192, 80), (1, 2, CHUNK + 64, 64), (1, 8, 1024, 40)]


@pytest.mark.parametrize("B,heads,N,d", KV_SHAPES)
def test_cross_attn_bwd_kv_matches_fp64_autograd(lib, B, heads, N, d):
    c = attn_case(B, heads, N, d, keys=CTX)
    got = run_kv(lib, c, B, heads, N, d)
    for name, g in zip(("dk", "dv"), got):
        assert torch.isfinite(g.float()).all(), name
        assert (g[:, CTX:] == 0).all(), name + ": rows 77 .. 79 must be exact zeros"
        err = G.rel_err(g[:, :CTX], c[name])
        print(f"cross_attn_bwd_kv B={B} heads={heads} N={N} d={d} {name}: {err:.3e}")
        G.within(err, 6e-3, what="cross_attn_bwd_kv " + name)


@pytest.mark.parametrize("B,heads,N,d", [(2, 2, 128, 40), (2, 1, 192, 80)])
def test_cross_attn_bwd_kv_batch_rows_are_single_calls(lib, B, heads, N, d):
    c = attn_case(B, heads, N, d, keys=CTX)
    got = run_kv(lib, c, B, heads, N, d)
    again = run_kv(lib, c, B, heads, N, d)
    for g, a in zip(got, again):
        assert torch.equal(g, a)                                  # two calls: the same bits
    for b in range(B):
        one = run_kv(lib, c, B, heads, N, d, rows=slice(b, b + 1))
        for g, o in zip(got, one):
            assert torch.equal(g[b:b + 1], o), b


def test_cross_attn_bwd_kv_rejects_bad_arguments(lib):
    buf = torch.zeros(1 << 18, dtype=dt(), device=G.dev())
    b = _lib.ptr(buf)

    def call(ldq=64, ldk=64, ldv=64, ldo=64, lddo=64, lddkv=64, B=1, N=64, heads=2, d=32, ws=b):
        return lib.hedit_k_cross_attn_bwd_kv(b, ldq, b, ldk, b, ldv, b, ldo, b, lddo, b, b, lddkv, B, N, heads, d, ws, None)

    assert call() == 0
    G.sync()
    for bad in (dict(N=96), dict(N=0), dict(d=48), dict(ldq=32), dict(ldk=32), dict(ldv=56), dict(lddo=60), dict(lddkv=32), dict(B=0),
                dict(ws=None)):
        assert call(**bad) == ERR_ARG, bad
    assert lib.hedit_k_cross_attn_bwd_kv_ws_bytes(0, 64, 2, 32) == 0


# ---------------------------------------------------------------------------------------------- the executor
class CtxNet(Net):
    """Net (tests/test_gpu_unet_grad.py) on a hedit_unet_create_grad_ctx handle, with the context backward"""

    def __init__(self, config, seed):
        from hedit.unet import UNet2DConditionModel, random_state_dict
        self.cfg = dict(config)
        self.hip = UNet2DConditionModel(self.cfg, device=G.dev(), grad="context")
        self.sd = random_state_dict(self.hip.param_shapes, seed)
        self.hip.load_state_dict(self.sd)
        self.lib, self.h = self.hip._lib, self.hip._h
        self.ws = None

    def backward_ctx(self, u, with_x=True):
        B = u.shape[0]
        dx = torch.full_like(u, float("nan")) if with_x else None
        dc = torch.full((B, CTX, self.cfg["cross_attention_dim"]), float("nan"), dtype=torch.float32, device=G.dev())
        _lib.check(self.lib.hedit_unet_backward_ctx(self.h, _lib.ptr(u), _lib.ptr(dx) if with_x else None, _lib.ptr(dc), _lib.ptr(self.ws), None))
        G.sync()
        return dx, dc


@pytest.fixture(scope="module")
def tiny():
    from hedit.unet import TINY_CONFIG
    return CtxNet(TINY_CONFIG, 0)


@pytest.fixture(scope="module")
def tiny_x():
    """the same network on a hedit_unet_create_grad handle"""
    from hedit.unet import TINY_CONFIG
    return Net(TINY_CONFIG, 0)


def test_d_ctx_matches_oracle_autograd(tiny):
    """d_ctx of hedit_unet_backward_ctx against torch.autograd of the fp32 oracle with respect to the context; the limit and the
    CPU measurement it comes from (bf16 autocast moves the oracle's own d_ctx by 2.704e-2 on exactly these inputs) are in the
    module docstring."""
    B, S, t = 2, 32, 501.0
    x, ctx, u = tiny.inputs(B, S, 30)
    cc = ctx.clone().requires_grad_(True)
    eps_want = tiny.om(x, torch.tensor(t), encoder_hidden_states=cc).sample
    (want,) = torch.autograd.grad((eps_want * u).sum(), cc)
    eps = tiny.keep(G.f32(x), t, G.f32(ctx))
    dx, dc = tiny.backward_ctx(G.f32(u))
    assert dc.shape == ctx.shape and torch.isfinite(dc).all() and torch.isfinite(dx).all()
    err = G.rel_err(dc, want)
    print(f"unet d_ctx B={B} S={S} t={t}: {err:.3e} (eps {G.rel_err(eps, eps_want.detach()):.3e})")
    G.within(err, TOL_DCTX, what="unet d_ctx")


def test_backward_ctx_bits(tiny, tiny_x):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(2, 32, 50))
    eps = tiny.keep(x, 501.0, ctx)
    dx, dc = tiny.backward_ctx(u)
    assert torch.equal(dx, tiny.backward(u))                       # hedit_unet_backward on the same handle and tape
    eps_x = tiny_x.keep(x, 501.0, ctx)
    assert torch.equal(eps_x, eps) and torch.equal(tiny_x.backward(u), dx)       # and on a create_grad handle
    none, dc0 = tiny.backward_ctx(u, with_x=False)                 # d_x = NULL: the same d_ctx
    assert none is None and torch.equal(dc0, dc)
    dx2, dc2 = tiny.backward_ctx(u)                                # a second backward on the same tape
    assert torch.equal(dx2, dx) and torch.equal(dc2, dc)
    for i in range(2):                                             # batch rows are single calls
        tiny.keep(x[i:i + 1].contiguous(), 501.0, ctx[i:i + 1].contiguous())
        dxi, dci = tiny.backward_ctx(u[i:i + 1].contiguous())
        assert torch.equal(dxi, dx[i:i + 1]) and torch.equal(dci, dc[i:i + 1]), i


def test_handles_and_workspace(tiny, tiny_x):
    lib = tiny.lib
    x, ctx, u = (G.f32(v) for v in tiny.inputs(1, 32, 95))
    tiny_x.keep(x, 501.0, ctx)
    dx = torch.empty_like(x)
    dc = torch.empty(1, CTX, 64, dtype=torch.float32, device=G.dev())
    assert lib.hedit_unet_backward_ctx(tiny_x.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(dc), _lib.ptr(tiny_x.ws), None) == ERR_STATE
    assert b"hedit_unet_create_grad_ctx" in lib.hedit_last_error()
    tiny_x.backward(u)                                             # the refusal left the tape alone
    assert lib.hedit_unet_grad_workspace_bytes(tiny_x.h, 1, 32, 32) == WS_TINY_1_32
    assert lib.hedit_unet_grad_workspace_bytes(tiny.h, 1, 32, 32) > WS_TINY_1_32       # also dK_all, dV_all, statistics, partials
    lib.hedit_unet_release(tiny.h)
    ws = tiny.workspace(1, 32)
    assert lib.hedit_unet_backward_ctx(tiny.h, _lib.ptr(u), _lib.ptr(dx), _lib.ptr(dc), _lib.ptr(ws), None) == ERR_STATE     # nothing kept
    assert b"hedit_unet_forward_keep" in lib.hedit_last_error()
    tiny.keep(x, 501.0, ctx)
    assert lib.hedit_unet_backward_ctx(tiny.h, _lib.ptr(u), _lib.ptr(dx), None, _lib.ptr(ws), None) == ERR_ARG               # no d_ctx


def test_facade_differentiates_the_context(tiny, tiny_x):
    x, ctx, u = (G.f32(v) for v in tiny.inputs(2, 32, 80))
    kw = {"use_controller": False}
    eps_c = tiny.keep(x, 401.0, ctx)
    want_x, want_c = tiny.backward_ctx(u)
    xx, cc = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    eps = tiny.hip(xx, torch.tensor(401), encoder_hidden_states=cc, cross_attention_kwargs=kw).sample
    assert eps.requires_grad and torch.equal(eps.detach(), eps_c)
    gx, gc = torch.autograd.grad((eps * u).sum(), (xx, cc))
    G.sync()
    assert torch.equal(gx, want_x) and torch.equal(gc, want_c)
    eps = tiny.hip(x, 401.0, encoder_hidden_states=cc, cross_attention_kwargs=kw).sample          # only the context requires grad
    assert eps.requires_grad
    (gc1,) = torch.autograd.grad((eps * u).sum(), cc)
    G.sync()
    assert torch.equal(gc1, want_c)
    eps = tiny.hip(xx, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw).sample        # only the sample does
    (gx1,) = torch.autograd.grad((eps * u).sum(), xx)
    assert torch.equal(gx1, want_x)
    e1 = tiny.hip(x, 401.0, encoder_hidden_states=cc, cross_attention_kwargs=kw).sample           # the ticket check, as before
    tiny.hip(x, 401.0, encoder_hidden_states=ctx, cross_attention_kwargs=kw)
    with pytest.raises(RuntimeError, match="dropped"):
        torch.autograd.grad(e1.sum(), cc)
    with pytest.raises(NotImplementedError, match="in the way"):                                  # context gradients under an editor
        tiny.hip._attention_editor = object()
        try:
            tiny.hip(x, 401.0, encoder_hidden_states=cc)
        finally:
            del tiny.hip._attention_editor
    with pytest.raises(NotImplementedError, match="encoder_hidden_states"):                       # grad=True refuses, as before
        tiny_x.hip(xx, 401.0, encoder_hidden_states=cc, cross_attention_kwargs=kw)
    with pytest.raises(ValueError, match="context"):
        from hedit.unet import TINY_CONFIG, UNet2DConditionModel
        UNet2DConditionModel(TINY_CONFIG, device=G.dev(), grad="ctx")


# ---------------------------------------------------------------------------------------------- one null-text update, and the driver
def _nt_pipeline(steps):
    from hedit.pipeline import HEditPipeline
    from hedit.scheduler import DDIMScheduler
    from hedit.unet import TINY_CONFIG
    hip = HEditPipeline.from_random(TINY_CONFIG, seed=0, device=G.dev(), text_layers=2, grad="context")
    hip.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    hip.scheduler.config.timestep_spacing = "leading"
    hip.scheduler.set_timesteps(steps)
    return hip


class Recorder:
    """bound to hedit.inversion.pnp_baselines.F, as tests/golden/make_golden_nt.py binds one to the reference module's"""

    def __init__(self):
        self.calls = []

    def mse_loss(self, a, b, *args, **kw):
        loss = torch.nn.functional.mse_loss(a, b, *args, **kw)
        self.calls.append((a, b, float(loss.detach())))
        return loss


class _FirstStepDone(Exception):
    pass


def _first_step(monkeypatch, optimization_steps, epsilon=1e-5):
    """the first step of nulltext_pnp on the HIP pipeline (TINY_CONFIG, 4 DDIM steps): register_time opens every step, and its
    second call ends the run -> (pipeline, t, x_rec, x_ori, the recorder of the loss calls, what the optimiser saw)"""
    from hedit.engine import HEditEngine
    from hedit.inversion import pnp_baselines as PB
    hip = _nt_pipeline(4)
    w0 = G.f32(hash_normal((1, 4, 32, 32), 123) * 0.8)
    _, zs, wts = HEditEngine(hip).ddim_inversion(w0, [SRC], 1.0)
    rec = Recorder()
    monkeypatch.setattr(PB, "F", rec)
    seen = {}
    adam = torch.optim.Adam

    class Spy(adam):                       # the embedding the loop optimises: its .grad is the HIP model's own d_ctx
        def __init__(self, params, **kw):
            params = list(params)
            seen.setdefault("emb", params[0])
            seen.setdefault("lr", kw["lr"])
            super().__init__(params, **kw)

    monkeypatch.setattr(torch.optim, "Adam", Spy)
    calls = []

    def tell_time(model, t):
        calls.append(t)
        if len(calls) == 2:
            raise _FirstStepDone

    with pytest.raises(_FirstStepDone):
        PB.nulltext_pnp(hip, xT=wts[4].contiguous(), xT_ori=wts[:5], etas=0.0, prompts=[SRC, TAR], cfg_scales=[1.0, CFG_TAR],
                        zs=zs[:4], optimization_steps=optimization_steps, epsilon=epsilon, register_time=tell_time)
    G.sync()
    return hip, hip.scheduler.timesteps[0], wts[4].contiguous(), wts[3], rec, seen


SRC, TAR, CFG_TAR = "a cat sitting on a bench", "a dog sitting on a bench", 7.5


def test_first_null_text_update_is_wired_to_the_context_gradient(monkeypatch):
    """One Adam update of nulltext_pnp on the HIP pipeline, checked for wiring.  (A multi-step loop is not compared with the
    oracle: Adam's first step is lr g / (|g| + 1e-8), a sign, so a last-bit change in a near-zero gradient element moves that
    element by 2 lr = 2e-2.)

    1. The update recomputed in fp64 from the HIP model's own d_ctx (the embedding's .grad): -lr g / (|g| + 1e-8).  The loop's
       value is the fp32 difference of two embeddings of magnitude < 4, so its error is half an fp32 ulp at 4 over the step,
       2^-22 / 1e-2 = 2.4e-5 per element: limit 5e-5 (relative L2).
    2. That d_ctx is the context gradient of the right cotangent: with c the eta = 0 reverse_step coefficient on eps, the
       cotangent recomputed in fp64 from the HIP model's own eps is 2 (pred - x_ori) / numel * c * (1 - cfg_tar); pushed through
       the facade (hedit_unet_backward_ctx) it gives the loop's d_ctx.  The two cotangents differ by fp32 rounding (autograd forms
       it in fp32, in another order), which the 16-bit roundings inside the backward pass on: the project's limit for linearity
       in the cotangent, 2e-2 (tests/test_gpu_vae.py), applies; the loss and pred themselves agree to fp32 rounding (1e-5)."""
    from hedit.engine import Schedule
    from hedit.inversion.inversion_utils import encode_text
    hip, t, x_rec, x_ori, rec, seen = _first_step(monkeypatch, 1)
    assert len(rec.calls) == 1 and seen["lr"] == 1e-2
    pred, x_ori_seen, loss = rec.calls[0]
    assert torch.equal(x_ori_seen.reshape(x_ori.shape), x_ori)
    null = encode_text(hip, [""] * 2)[:1]
    emb, g = seen["emb"].detach(), seen["emb"].grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0 and float(emb.abs().max()) < 4.0
    want = -1e-2 * g.double() / (g.double().abs() + 1e-8)
    err = G.rel_err((emb - null).double(), want)
    print(f"null-text update vs fp64 recomputation from the loop's d_ctx: {err:.3e}")
    assert err < 5e-5, err
    kw = {"use_controller": False, "use_editor": False}
    with torch.no_grad():
        e_c = hip.unet(x_rec, t, encoder_hidden_states=encode_text(hip, [SRC, TAR])[:1], cross_attention_kwargs=kw).sample
    cc = null.clone().requires_grad_(True)
    e_u = hip.unet(x_rec, t, encoder_hidden_states=cc, cross_attention_kwargs=kw).sample
    S = Schedule(hip.scheduler)
    a_t, a_p = float(S.ab[int(t)]), float(S.ab_prev(int(t)))
    c = (1 - a_p) ** 0.5 - a_p ** 0.5 * (1 - a_t) ** 0.5 / a_t ** 0.5
    e64 = e_u.detach().double() + CFG_TAR * (e_c.double() - e_u.detach().double())
    pred64 = a_p ** 0.5 * (x_rec.double() - (1 - a_t) ** 0.5 * e64) / a_t ** 0.5 + (1 - a_p) ** 0.5 * e64
    assert G.rel_err(pred, pred64) < 1e-5 and abs(loss - float(((pred64 - x_ori.double()) ** 2).mean())) < 1e-5 * loss
    cot = (2.0 * (pred64 - x_ori.double()) / pred64.numel() * c * (1.0 - CFG_TAR)).float().contiguous()
    (g_c,) = torch.autograd.grad(e_u, cc, cot)
    G.sync()
    e_g = G.rel_err(g_c, g)
    print(f"null-text update: d_ctx of the fp64 cotangent vs the loop's d_ctx {e_g:.3e}")
    G.within(e_g, 2e-2, what="null-text cotangent")


def test_inner_loss_decreases_where_the_reference_does(monkeypatch):
    """tests/golden/g24_nulltext.json, case `full` (2 updates per step): in the reference's own run the last inner loss of step 0
    is below its first.  The HIP loop with the same settings on its own toy: the same holds for its step 0."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "g24_nulltext.json")) as f:
        case = [c for c in json.load(f)["cases"] if c["decreases"]][0]
    assert case["losses"][0][-1] < case["losses"][0][0] and case["updates"][0] == case["optimization_steps"] > 1
    rec = _first_step(monkeypatch, case["optimization_steps"], case["epsilon"])[4]
    losses = [c[2] for c in rec.calls]
    print("inner losses of step 0:", losses)
    assert len(losses) == case["optimization_steps"] and losses[-1] < losses[0]


def _nt_driver():
    spec = importlib.util.spec_from_file_location("hedit_main_nt", os.path.join(ROOT, "h-edit_amd", "main_nt.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_nt_driver_writes_edited_images(tmp_path):
    """nt_pnp from a PIE-Bench-style mapping file to non-constant 256 x 256 PNGs, and --batch 2 (lock-step: one embedding, one
    optimiser, one loss per image): byte-identical files; other modes are refused with the driver that runs them"""
    import numpy as np
    from PIL import Image
    from helpers.datasets import pie_dataset as _dataset
    d = _dataset(tmp_path)
    common = ["--data_path", str(d), "--random_init", "--tiny", "--num_diffusion_steps", "4", "--edit_category_list", "0", "1",
              "--mode", "nt_pnp", "--pnp_f_t", "0.5", "--pnp_attn_t", "0.75"]
    one = _nt_driver().main(common + ["--output_path", str(tmp_path / "r1")])
    assert len(one) == 2                           # category 7 filtered out
    for p in one:
        sub = os.path.relpath(p, str(tmp_path / "r1")).split(os.sep)[0]
        assert sub.startswith("nt_pnp_total_steps_4_skip_0_implicit_False_eta_0.0_") and sub.endswith("_f_t_0.5_attn_t_0.75_"), sub
        im = np.array(Image.open(p))
        assert im.shape == (256, 256, 3) and im.std() > 0
    two = _nt_driver().main(common + ["--output_path", str(tmp_path / "r2"), "--batch", "2"])
    assert len(two) == 2
    for a, b in zip(sorted(one), sorted(two)):
        assert os.path.basename(a) == os.path.basename(b)
        assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b)))
    for mode, where in (("nmg_pnp", "main_nmg.py"), ("np_pnp", "main_baselines.py")):
        with pytest.raises(NotImplementedError) as ei:
            _nt_driver().main(common[:-5] + [mode])
        assert mode in str(ei.value) and where in str(ei.value)
