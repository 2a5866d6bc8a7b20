"""UNet2DConditionModel facade over the native HIP executor (csrc/unet.hip).

Exposes the surface the reference uses of diffusers' UNet:
``unet(sample, timestep, encoder_hidden_states=, cross_attention_kwargs=).sample`` /
``["sample"]`` (text-guided/inversion/p2p_h_edit.py:613, ddpm_inversion.py:130),
``in_channels`` / ``sample_size`` (ddpm_inversion.py:29-31), ``attn_processors`` /
``set_attn_processor`` (p2p/ptp_utils.py:280,294), ``zero_grad`` (main_p2p.py:277), and the
diffusers state_dict key names for weights.

The attention processors are markers: the Prompt-to-Prompt edit itself runs inside the HIP
attention kernels, driven by a per-call plan compiled from the registered controller
(hedit/p2p/ptp_classes.py).  A controller that is NOT one of hedit's (any object callable as the
reference's ``controller(attention_probs, is_cross, place_in_unet, save_attn)``,
p2p/ptp_utils.py:98-106, p2p/ptp_classes.py:91-108) is served by the hook path of the executor
(``hedit_unet_set_attn_hook``): every attention layer materialises its probabilities, the controller
sees and may rewrite them in place, the executor multiplies what comes back with V.  Slow (fp32
probabilities through HBM), same protocol.

``UNet2DConditionModel(config, device, grad=True)`` also carries the input-gradient weights (hedit_unet_create_grad):
whenever grad mode is on and ``sample.requires_grad``, a PLAIN pass (``use_controller=False`` or no controller registered,
no attention editor) is an autograd node whose backward is the executor's input-gradient pass -- what Noise Map Guidance
differentiates (text-guided/inversion/p2p_baselines.py:251-268).  The gradient is with respect to the sample only.

``grad="context"`` builds the handle of hedit_unet_create_grad_ctx instead: the same node then also answers for
``encoder_hidden_states`` when that requires grad (hedit_unet_backward_ctx) -- what null-text inversion optimises
(text-guided/inversion/pnp_baselines.py:134-236).  Nothing else changes; ``grad=True`` still refuses such a context.
"""
import ctypes as C
import hashlib
import math

import torch

from . import _lib
from . import native
from .native import NativeOwner

SD15_CONFIG = dict(in_channels=4, out_channels=4, sample_size=64,
                   block_out_channels=(320, 640, 1280, 1280),
                   down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D",
                                     "CrossAttnDownBlock2D", "DownBlock2D"),
                   up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D",
                                   "CrossAttnUpBlock2D"),
                   layers_per_block=2, cross_attention_dim=768, attention_head_dim=8,
                   norm_num_groups=32)

# three levels at 32x32 latents, keeps SD's stored-cross-map inventory (tests / smoke)
TINY_CONFIG = dict(in_channels=4, out_channels=4, sample_size=32,
                   block_out_channels=(64, 128, 128),
                   down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                   up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                   layers_per_block=2, cross_attention_dim=64, attention_head_dim=2,
                   norm_num_groups=32)


class UNetOutput(dict):
    @property
    def sample(self):
        return self["sample"]


class AttnProcessor:
    """Plain attention (no controller).  Marker only."""
    controller = None


def random_state_dict(param_shapes, seed=0):
    """Synthetic weights (no checkpoints exist offline): W ~ N(0, 1/fan_in),
    small random biases / norm affine terms.  Each tensor is seeded by (seed, name), so the
    result does not depend on iteration order."""
    sd = {}
    for name, shape in param_shapes.items():
        hsh = hashlib.sha256(f"{seed}:{name}".encode()).digest()
        g = torch.Generator().manual_seed(int.from_bytes(hsh[:7], "little"))
        if len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[name] = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        elif "norm" in name and name.endswith("weight"):
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif "norm" in name:
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        else:
            sd[name] = 0.02 * torch.randn(shape, generator=g)
    return sd


class _EpsGrad(torch.autograd.Function):
    """eps = unet(sample, t, ctx) with the forward's tape kept in the model's gradient workspace; backward = the executor's
    vector-Jacobian product with respect to whichever of (sample, ctx) ``needs_input_grad`` asks for (ctx: a
    ``grad="context"`` model, hedit_unet_backward_ctx).  The tape stays until the model's next call, so ``retain_graph=True`` and a second backward
    work; a backward after the model has run again is an error, not another forward's gradient (the ticket check of
    hedit/diffusion/diffusion.py)."""

    @staticmethod
    def forward(ctx, sample, enc, model, t):
        ctx.model = model
        ctx.ticket, eps = model._keep(sample.detach(), t, enc)
        ctx.shape = sample.shape
        ctx.enc_shape = enc.shape
        return eps

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        if m._ticket != ctx.ticket:
            raise RuntimeError("hedit.UNet2DConditionModel: the kept forward of this graph was dropped by a later model call")
        g = g.detach().to(dtype=torch.float32).contiguous()
        want_x, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=m.device) if want_x else None
        dc = torch.empty(ctx.enc_shape, dtype=torch.float32, device=m.device) if want_c else None
        with torch.cuda.device(m.device):
            if want_c:
                _lib.check(m._lib.hedit_unet_backward_ctx(m._h, _lib.ptr(g), _lib.ptr(dx) if want_x else None, _lib.ptr(dc),
                                                          _lib.ptr(m._gws), _lib.cur_stream()))
            elif want_x:
                _lib.check(m._lib.hedit_unet_backward(m._h, _lib.ptr(g), _lib.ptr(dx), _lib.ptr(m._gws), _lib.cur_stream()))
        return dx, dc, None, None


class UNetContext(NativeOwner):
    """A bound text context (hedit_unet_context, include/hedit.h): the padded bf16 rows of ``ctx`` and their attn2 key / value
    projections for every transformer block, computed once by ``UNet2DConditionModel.make_context`` and handed to
    ``forward_raw(ctx=...)`` in place of the tensor.  A SNAPSHOT: later changes to the tensor (or to the model's weights) do not
    reach it.  Owns device memory of its own (4 MB per row for SD-1.5); ``close()`` or dropping the object frees it, before or
    after the model."""
    _family, _finalizes = "unet_context", False

    def __init__(self, model, ctx):
        rows, _, dim = ctx.shape
        if ctx.dtype != torch.float32 or ctx.shape != (rows, 77, model.config["cross_attention_dim"]):
            raise ValueError(f"the context rows must be float32 (B, 77, {model.config['cross_attention_dim']}), got "
                             f"{ctx.dtype} {tuple(ctx.shape)}")
        ctx = ctx.detach().to(model.device).contiguous()
        lib, h = model._lib, C.c_void_p()
        with native._device_ctx(model.device):
            _lib.check(lib.hedit_unet_context_create(model._h, _lib.ptr(ctx), rows, _lib.cur_stream(), C.byref(h)))
            native._sync_stream()      # the launches read `ctx`: keep it alive until they ran
        self.rows = rows
        self._h, self._lib, self._h_device = h, lib, model.device

    close = NativeOwner._native_release


class UNet2DConditionModel(NativeOwner):
    _family, _finalizes = "unet", False
    _tickets = 0      # kept forwards so far, over all models: a ticket is never reused

    def __init__(self, config=None, device="cuda:0", grad=False):
        cfg = dict(SD15_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("hedit.UNet2DConditionModel runs on the GPU only (HIP kernels)")
        self.in_channels = cfg["in_channels"]
        self.sample_size = cfg["sample_size"]
        c = _lib.UnetCfg()
        c.in_channels, c.out_channels, c.sample_size = cfg["in_channels"], cfg["out_channels"], cfg["sample_size"]
        ch = list(cfg["block_out_channels"])
        c.n_levels = len(ch)
        for i, v in enumerate(ch):
            c.block_out_channels[i] = v
            c.down_has_attn[i] = int(cfg["down_block_types"][i].startswith("CrossAttn"))
            c.up_has_attn[i] = int(cfg["up_block_types"][i].startswith("CrossAttn"))
        c.layers_per_block = cfg["layers_per_block"]
        c.cross_attention_dim = cfg["cross_attention_dim"]
        c.heads = cfg["attention_head_dim"]
        c.norm_num_groups = cfg["norm_num_groups"]
        self._cfg_struct = c
        if isinstance(grad, str) and grad != "context":
            raise ValueError(f'grad must be False, True or "context", got {grad!r}')
        self._native_build(self.device, None, c, create="create_grad_ctx" if grad == "context" else "create_grad" if grad else "create")
        self.grad = bool(grad)
        self.grad_context = grad == "context"      # the handle also differentiates encoder_hidden_states
        self._ticket = 0          # identifies the kept forward; 0 = none
        self._gws = None          # the tape's workspace (hedit_unet_grad_workspace_bytes)
        self.param_shapes = self._native_param_shapes()
        # parameters the executor keeps as unscaled bf16 copies (hedit.dist sends those as bf16)
        self.bf16_exact = {name for i, name in enumerate(self.param_shapes) if self._lib.hedit_unet_param_bf16_exact(self._h, i)}
        self._procs = {n: AttnProcessor() for n in self._processor_names()}
        self.heads = cfg["attention_head_dim"]

    # ---------------------------------------------------------------- weights
    load_state_dict = NativeOwner._native_load

    def init_random(self, seed=0):
        sd = random_state_dict(self.param_shapes, seed)
        self.load_state_dict(sd)
        return sd

    def zero_grad(self, *a, **k):
        return None

    # ---------------------------------------------------------------- processor registry
    def _processor_names(self):
        cfg = self.config
        names = []
        L = cfg["layers_per_block"]
        for i, t in enumerate(cfg["down_block_types"]):
            if t.startswith("CrossAttn"):
                for j in range(L):
                    for a in ("attn1", "attn2"):
                        names.append(f"down_blocks.{i}.attentions.{j}.transformer_blocks.0.{a}.processor")
        for a in ("attn1", "attn2"):
            names.append(f"mid_block.attentions.0.transformer_blocks.0.{a}.processor")
        for i, t in enumerate(cfg["up_block_types"]):
            if t.startswith("CrossAttn"):
                for j in range(L + 1):
                    for a in ("attn1", "attn2"):
                        names.append(f"up_blocks.{i}.attentions.{j}.transformer_blocks.0.{a}.processor")
        return names

    @property
    def attn_processors(self):
        return dict(self._procs)

    def set_attn_processor(self, procs):
        if not isinstance(procs, dict):
            procs = {k: procs for k in self._procs}
        for k, p in procs.items():
            if k not in self._procs:
                raise KeyError(f"unknown attention processor name {k}")
            if not hasattr(p, "controller"):
                raise TypeError(
                    f"{type(p).__name__}: a processor is identified by its .controller (None = plain attention, a hedit "
                    "controller = in-kernel edit, any other callable = hooked through hedit_unet_set_attn_hook); processor "
                    "objects that re-implement the attention body itself cannot be run -- the body is the HIP kernels")
            c = p.controller
            if c is not None and not hasattr(c, "_plan") and not callable(c):      # (hedit's own are callable too)
                raise TypeError(f"{type(c).__name__}: a foreign controller must be callable as "
                                "controller(attention_probs, is_cross, place_in_unet, save_attn)")
            self._procs[k] = p

    def _controller(self):
        ctrls = {id(p.controller): p.controller for p in self._procs.values() if p.controller is not None}
        if not ctrls:
            return None
        if len(ctrls) != 1 or any(p.controller is None for p in self._procs.values()):
            raise RuntimeError("all attention layers must share one controller "
                               "(use hedit.p2p.ptp_utils.register_attention_control)")
        return next(iter(ctrls.values()))

    # ---------------------------------------------------------------- geometry helpers
    def store_layers(self, height, width):
        """[(tokens, place)] of the cross-attention layers whose maps are stored (<= 32*32 tokens),
        in call order; place in {'down','mid','up'}."""
        n = self._lib.hedit_unet_num_store_layers(self._h, height, width)
        out = []
        tok, pl = C.c_int(), C.c_int()
        for i in range(n):
            _lib.check(self._lib.hedit_unet_store_layer_info(self._h, height, width, i, C.byref(tok), C.byref(pl)))
            out.append((tok.value, ("down", "mid", "up")[pl.value]))
        return out

    def _workspace(self, B, H, W):
        need = self._lib.hedit_unet_workspace_bytes(self._h, B, H, W)
        if need == 0:
            raise _lib.HipError("workspace planning failed: " + self._lib.hedit_last_error().decode())
        return self._grow("_ws", need, self.device)

    # ---------------------------------------------------------------- sampled launch timing
    PROF_KINDS = ("conv3x3_gemm", "linear_gemm", "self_attn", "cross_attn", "norm", "other")

    def prof_enable(self, on, max_records=8192):
        _lib.check(self._lib.hedit_prof_enable(self._h, int(on), max_records))

    def prof_reset(self):
        _lib.check(self._lib.hedit_prof_reset(self._h))

    def prof_collect(self):
        """{kind: (total_ms, total_flops, launches)}; synchronises the device first."""
        torch.cuda.synchronize(self.device)
        out = {}
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        for i, k in enumerate(self.PROF_KINDS):
            _lib.check(self._lib.hedit_prof_collect(self._h, i, C.byref(ms), C.byref(fl), C.byref(n)))
            out[k] = (ms.value, fl.value, n.value)
        return out

    def prof_collect_bytes(self):
        """{kind: algorithmic HBM bytes of the sampled launches} (operands read once, results written once)."""
        out = {}
        b = C.c_double()
        for i, k in enumerate(self.PROF_KINDS):
            _lib.check(self._lib.hedit_prof_collect_bytes(self._h, i, C.byref(b)))
            out[k] = b.value
        return out

    def prof_records(self, max_rows=16384):
        """numpy (n, 8): kind, ms, flops, bytes, M, N, K, tag per sampled launch, in launch order."""
        import numpy as np
        torch.cuda.synchronize(self.device)
        rows = np.zeros((max_rows, 8), dtype=np.float64)
        n = C.c_int()
        _lib.check(self._lib.hedit_prof_records(self._h, rows.ctypes.data_as(C.POINTER(C.c_double)), max_rows, C.byref(n)))
        return rows[:n.value]

    # ---------------------------------------------------------------- forward
    def make_context(self, ctx_rows):
        """ctx_rows fp32 (B,77,D) -> a UNetContext for ``forward_raw(ctx=...)``: the per-call context projections, once"""
        return UNetContext(self, ctx_rows)

    def forward_raw(self, sample, t, ctx, plan=None, out=None, row_latent=None):
        """sample fp32 (B,C,H,W) cuda, t python float, ctx fp32 (B,77,D) cuda or a UNetContext of B rows (make_context: the
        same bits without the per-call projections), plan: _lib.P2PPlan.
        row_latent (sequence of B ints): ``sample`` then holds only the DISTINCT latents and row r evaluates
        ``sample[row_latent[r]]`` under ``ctx[r]`` -- the bits of the call on ``sample[row_latent]``, with the part of the
        network in front of the first cross-attention run once per latent where the executor may (hedit_unet_forward_shared)."""
        B, Cc, H, W = sample.shape
        if row_latent is not None:
            B = len(row_latent)
        bound = isinstance(ctx, UNetContext)
        if sample.dtype != torch.float32 or (not bound and ctx.dtype != torch.float32):
            raise TypeError("sample and encoder_hidden_states must be float32")
        if bound:
            if ctx._h is None:
                raise _lib.HipError("the UNetContext was closed")
            ctx_arg = ctx._h
        else:
            if ctx.shape != (B, 77, self.config["cross_attention_dim"]):
                raise ValueError(f"encoder_hidden_states must be ({B}, 77, {self.config['cross_attention_dim']}), "
                                 f"got {tuple(ctx.shape)}")
            ctx = ctx.contiguous()
            ctx_arg = _lib.ptr(ctx)
        sample = sample.contiguous()
        if out is None:
            out = torch.empty(B, self.config["out_channels"], H, W, dtype=torch.float32, device=sample.device)
        ws = self._workspace(B, H, W)
        if row_latent is None:
            fwd = self._lib.hedit_unet_forward_bound if bound else self._lib.hedit_unet_forward
            _lib.check(fwd(
                self._h, _lib.ptr(sample), C.c_float(float(t)), ctx_arg, B, H, W,
                C.byref(plan) if plan is not None else None, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                _lib.cur_stream()))
            return out
        if sample.data_ptr() % 16:
            sample = sample.clone()
        fwd = self._lib.hedit_unet_forward_shared_bound if bound else self._lib.hedit_unet_forward_shared
        _lib.check(fwd(
            self._h, _lib.ptr(sample), sample.shape[0], (C.c_int * B)(*row_latent), C.c_float(float(t)), ctx_arg, B, H, W,
            C.byref(plan) if plan is not None else None, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
            _lib.cur_stream()))
        return out

    # ---------------------------------------------------------------- input gradient
    def _release(self):
        if self._ticket:
            self._lib.hedit_unet_release(self._h)
            self._ticket = 0

    def _keep(self, sample, t, ctx):
        """plain forward that leaves its tape in the gradient workspace -> (the ticket a backward must present, eps)"""
        sample, ctx = sample.contiguous(), ctx.detach().contiguous()
        B, _, H, W = sample.shape
        if ctx.shape != (B, 77, self.config["cross_attention_dim"]):
            raise ValueError(f"encoder_hidden_states must be ({B}, 77, {self.config['cross_attention_dim']}), got {tuple(ctx.shape)}")
        need = self._lib.hedit_unet_grad_workspace_bytes(self._h, B, H, W)
        if need == 0:
            raise _lib.HipError("gradient workspace planning failed: " + self._lib.hedit_last_error().decode())
        self._grow("_gws", need, self.device)
        eps = torch.empty(B, self.config["out_channels"], H, W, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.hedit_unet_forward_keep(self._h, _lib.ptr(sample), C.c_float(float(t)), _lib.ptr(ctx), B, H, W,
                                                         _lib.ptr(eps), _lib.ptr(self._gws), self._gws.numel(), _lib.cur_stream()))
        UNet2DConditionModel._tickets += 1
        self._ticket = UNet2DConditionModel._tickets
        return self._ticket, eps

    _HOOK_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)

    def forward_hooked(self, sample, t, ctx, controller, save_attn=True, out=None):
        """One UNet call with a foreign (host-language) controller: ``controller(attention_probs, is_cross,
        place_in_unet, save_attn)`` is called once per attention layer, in execution order, with the reference's tensor
        (fp32 [batch * heads, queries, keys], a fresh tensor per layer like the reference's, so a controller may keep it);
        in-place changes go into the product with V, the return value is ignored (ptp_utils.py:100-106)."""
        B, _, H, W = sample.shape
        state = {"exc": None}
        places = ("down", "mid", "up")

        def cb(_user, probs, bh, nq, nk, is_cross, place, _layer, _stream):
            try:
                off = int(probs) - self._ws.data_ptr()
                view = self._ws[off:off + bh * nq * nk * 4].view(torch.float32).view(bh, nq, nk)
                attn = view.clone()
                controller(attn, bool(is_cross), places[place], save_attn)
                view.copy_(attn)
                return 0
            except BaseException as e:      # noqa: BLE001  (must not unwind through the C frames)
                state["exc"] = e
                return 1

        fn = self._HOOK_T(cb)
        _lib.check(self._lib.hedit_unet_set_attn_hook(self._h, C.cast(fn, C.c_void_p), None))
        try:
            try:
                return self.forward_raw(sample, t, ctx, None, out)      # (the workspace is sized with the hook set)
            except _lib.HipError:
                if state["exc"] is not None:
                    raise state["exc"]
                raise
        finally:
            _lib.check(self._lib.hedit_unet_set_attn_hook(self._h, None, None))

    def forward(self, sample, timestep=None, encoder_hidden_states=None, cross_attention_kwargs=None,
                return_dict=True):
        kw = dict(cross_attention_kwargs or {})
        use_controller = kw.pop("use_controller", True)
        save_attn = kw.pop("save_attn", True)
        use_editor = kw.pop("use_editor", True)          # MasaCtrl's switch (masactrl_utils.py:40)
        if kw:
            raise TypeError(f"unsupported cross_attention_kwargs {sorted(kw)}")
        if isinstance(timestep, torch.Tensor):
            tt = timestep.reshape(-1)
            if tt.numel() > 1 and not bool((tt == tt[0]).all()):
                raise NotImplementedError("per-sample timesteps: the batch must share one timestep")
            t = float(tt[0])
        else:
            t = float(timestep)
        sample = sample.to(device=self.device, dtype=torch.float32)
        ctx = encoder_hidden_states.to(device=self.device, dtype=torch.float32)
        controller = self._controller() if use_controller else None
        if controller is None and use_editor:
            # an attention editor registered on the UNet (MasaCtrl: regiter_attention_editor_diffusers; Plug-and-Play:
            # register_attention_control_efficient / register_conv_control_efficient)
            controller = getattr(self, "_attention_editor", None)
        if self.grad:
            self._release()
            ctx_grad = torch.is_grad_enabled() and encoder_hidden_states.requires_grad
            if ctx_grad and not self.grad_context:
                raise NotImplementedError("the gradient with respect to encoder_hidden_states (null-text inversion) is not "
                                          "implemented on this model: the input-gradient pass of grad=True differentiates the "
                                          "sample only (build the model with grad=\"context\")")
            if torch.is_grad_enabled() and (sample.requires_grad or ctx_grad):
                if controller is not None:
                    what = "an attention editor" if controller is getattr(self, "_attention_editor", None) else "a registered controller"
                    raise NotImplementedError(f"{what} ({type(controller).__name__}) is in the way: the input-gradient pass differentiates the plain network "
                                              "only (pass cross_attention_kwargs={'use_controller': False, 'use_editor': False})")
                return UNetOutput(sample=_EpsGrad.apply(sample, ctx, self, t))
        from .p2p.ptp_classes import runs_in_python
        if runs_in_python(controller):
            return UNetOutput(sample=self.forward_hooked(sample, t, ctx, controller, save_attn))
        plan = None
        if controller is not None:
            plan = controller._plan(self, sample.shape[0], sample.shape[2], sample.shape[3], save_attn)
        eps = self.forward_raw(sample, t, ctx, plan)
        if controller is not None:
            controller._after_pass(save_attn)
        return UNetOutput(sample=eps)

    __call__ = forward
