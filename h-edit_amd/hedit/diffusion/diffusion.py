"""The face model's pixel-space DDPM UNet on the native HIP executor (csrc/ddpm.hip) behind the interface
of the reference's ``face-swapping/diffusion/diffusion.py::Model`` (:192-341): constructed from the
same config keys, called as ``model(x, t)`` with ``x`` (n, 3, S, S) and ``t`` the (n,) float tensor of
equal timesteps the reference passes (h_edit_R.py:70-71; a scalar works too) -> eps (n, 3, S, S) fp32;
attributes ``in_channels`` / ``resolution`` read by the SDE inversion (sde_inversion.py:32-33);
state_dict key names of the reference class.  GPU only -- there is no eager path.

``Model(config, device, grad=True)`` also carries the input-gradient weights (hedit_ddpm_create_grad): whenever grad
mode is on and ``x.requires_grad`` the call is an autograd node whose backward is the executor's input-gradient pass
(what the face task's Edit Friendly mode differentiates, face-swapping/inversion/ef.py:64-66,95,106).  Weights and ``t``
take no gradient."""
import torch

from .. import _lib
from ..native import NativeOwner
from ..unet import random_state_dict

# the CelebA-HQ 256 x 256 model the reference loads (face-swapping/main_edit.py: config of the DDPM checkpoint)
CELEBA_HQ_CONFIG = dict(type="simple", in_channels=3, out_ch=3, ch=128, ch_mult=(1, 1, 2, 2, 4, 4), num_res_blocks=2,
                        attn_resolutions=(16,), dropout=0.0, image_size=256, resamp_with_conv=True,
                        num_diffusion_timesteps=1000)
TINY_DDPM_CONFIG = dict(type="simple", in_channels=3, out_ch=3, ch=64, ch_mult=(1, 2), num_res_blocks=1,
                        attn_resolutions=(16,), dropout=0.0, image_size=32, resamp_with_conv=True,
                        num_diffusion_timesteps=1000)


class _EpsGrad(torch.autograd.Function):
    """eps = model(x, t) with the forward's tape kept in the model's workspace; backward = the executor's vector-Jacobian
    product.  The tape stays until the model's next call, so ``retain_graph=True`` and a second backward work (ef.py:95,
    :106); a backward after the model has run again is an error, not a wrong gradient."""

    @staticmethod
    def forward(ctx, x, model, t0):
        ctx.model = model
        ctx.ticket, eps = model._keep(x.detach(), t0)
        ctx.shape = x.shape
        return eps

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        if m._ticket != ctx.ticket:
            raise RuntimeError("hedit.diffusion.Model: the kept forward of this graph was dropped by a later model call")
        g = g.detach().to(dtype=torch.float32).contiguous()
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=m.device)
        with torch.cuda.device(m.device):
            _lib.check(m._lib.hedit_ddpm_backward(m._h, _lib.ptr(g), _lib.ptr(dx), _lib.ptr(m._ws), _lib.cur_stream()))
        return dx, None, None


class Model(NativeOwner):
    _family, _finalizes = "ddpm", False
    # the timestep is a launch parameter: a (n,) tensor that still lives on the host is read without a device
    # synchronisation, so callers that know t on the host (the loops do) should not move it to the GPU first
    accepts_host_timesteps = True
    _tickets = 0      # kept forwards so far, over all models: a ticket is never reused

    def __init__(self, config=None, device="cuda:0", grad=False):
        cfg = dict(CELEBA_HQ_CONFIG)
        cfg.update(config or {})
        if not cfg.get("resamp_with_conv", True):
            raise NotImplementedError("resamp_with_conv=False (average-pool resampling) is not built")
        if cfg.get("type", "simple") == "bayesian":
            raise NotImplementedError("the 'bayesian' variant's logvar parameter is unused by the sampler and not built")
        self.config = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("hedit.diffusion.Model runs on the GPU only (HIP kernels)")
        self.in_channels = cfg["in_channels"]
        self.resolution = cfg["image_size"]
        self.ch = cfg["ch"]
        c = _lib.DdpmCfg()
        c.in_channels, c.out_ch, c.ch = cfg["in_channels"], cfg["out_ch"], cfg["ch"]
        mult = list(cfg["ch_mult"])
        c.n_levels = len(mult)
        res = cfg["image_size"]
        for i, m in enumerate(mult):
            c.ch_mult[i] = m
            c.attn_level[i] = int(res in tuple(cfg["attn_resolutions"]))
            if i != len(mult) - 1:
                res //= 2
        c.num_res_blocks, c.image_size = cfg["num_res_blocks"], cfg["image_size"]
        self._native_build(self.device, None, c, create="create_grad" if grad else "create")
        self.grad = bool(grad)
        self._ticket = 0          # identifies the kept forward; 0 = none
        self.param_shapes = self._native_param_shapes()

    # ---------------------------------------------------------------- weights
    def load_state_dict(self, sd, strict=True):
        return self._native_load({k: v for k, v in sd.items() if k != "logvar"}, strict)

    def init_random(self, seed=0):
        sd = random_state_dict(self.param_shapes, seed)
        self.load_state_dict(sd)
        return sd

    # the reference toggles these on the module; nothing to do for an inference-only executor
    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device:
            raise RuntimeError("the HIP executor is bound to its creation device")
        return self

    # ---------------------------------------------------------------- forward
    def __call__(self, x, t):
        return self.forward(x, t)

    def forward(self, x, t):
        assert x.shape[2] == x.shape[3] == self.resolution
        t0 = self._timestep(t)
        if self.grad:
            self._release()
            if torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad:
                return _EpsGrad.apply(x.to(device=self.device, dtype=torch.float32), self, t0)
        with torch.no_grad():
            return self._forward(x, t0)

    @staticmethod
    def _timestep(t):
        if torch.is_tensor(t):
            tv = t.detach().float().reshape(-1)
            t0 = float(tv[0])
            if tv.numel() > 1 and not bool((tv == tv[0]).all()):
                raise NotImplementedError("one timestep per call (the reference passes ones(n) * t)")
        else:
            t0 = float(t)
        return t0

    def _workspace(self, need, what):
        if need == 0:
            raise RuntimeError(what + " failed: " + self._lib.hedit_last_error().decode())
        self._grow("_ws", need, self.device)

    def _release(self):
        if self._ticket:
            self._lib.hedit_ddpm_release(self._h)
            self._ticket = 0

    def _keep(self, x, t0):
        """forward that leaves its tape in the workspace -> (the ticket a backward must present, eps)"""
        x = x.contiguous()
        B = x.shape[0]
        self._workspace(self._lib.hedit_ddpm_grad_workspace_bytes(self._h, B), "hedit_ddpm_grad_workspace_bytes")
        eps = torch.empty(B, self.config["out_ch"], self.resolution, self.resolution, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.hedit_ddpm_forward_keep(self._h, _lib.ptr(x), t0, B, _lib.ptr(eps), _lib.ptr(self._ws),
                                                         self._ws.numel(), _lib.cur_stream()))
        Model._tickets += 1
        self._ticket = Model._tickets
        return self._ticket, eps

    def _forward(self, x, t0):
        x = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        B = x.shape[0]
        self._workspace(self._lib.hedit_ddpm_workspace_bytes(self._h, B), "hedit_ddpm_workspace_bytes")
        out = torch.empty(B, self.config["out_ch"], self.resolution, self.resolution, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.hedit_ddpm_forward(self._h, _lib.ptr(x), t0, B, _lib.ptr(out), _lib.ptr(self._ws),
                                                    self._ws.numel(), _lib.cur_stream()))
        return out
