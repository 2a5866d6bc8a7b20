"""Structure Distance on the native executor (``hedit_dino_*`` of libhedit_hip.so, csrc/dino.hip): the metric the PIE-Bench
evaluator reports in its ``structure_distance`` / ``structure_distance_unedit_part`` / ``structure_distance_edit_part``
columns -- the reference's text-guided/evaluation/matrics_calculator.py:12-246,390-410 read literally:

1. both images as float32 arrays in 0...255 (NOT divided by 255), times their masks, laid out (1, 3, H, W);
2. ``Resize(224, max_size=480)`` on a tensor under torchvision 0.14.1 = bilinear, align_corners=False, NO antialias, then
   ``Normalize(imagenet mean, std)`` applied to those 0...255 values (both quirks kept: the published numbers come from them);
3. DINO ``dino_vitb8``; the keys of block 11, (heads, tokens, 64) concatenated per token to (tokens, 768);
4. ``S = K K^T / clamp(|k_i| |k_j|, min=1e-8)``;
5. ``mean((S_a - S_b)^2)``.

The network is the public DINO ViT (facebookresearch/dino vision_transformer.py).  PARITY UNPINNED against the published
network: no DINO code or weights exist offline and the reference tree holds no vector for this metric; what the tests check
is the native executor against a torch restatement of this description (tests/helpers/dino_ref.py).

Nothing is ever fetched and ``torch.hub`` is never called: weights come from a local file or from seeded stand-in values,
and there is no torch forward -- ``DinoNet`` is a parameter container, CPU tensors raise.  Square images only; a checkpoint
whose ``pos_embed`` does not fit the resolution is refused (positional-embedding interpolation is out of scope).
"""
import os
import re

import numpy as np
import torch

from .native import NativeOwner

MAX_PAIRS = 64            # HEDIT_DINO_MAX_PAIRS of include/hedit.h
MAX_TOKENS = 1025         # the executor's cap (csrc/dino.hip LMAX)
_BLOCK = re.compile(r"^blocks\.(\d+)\.(.+)$")
_WHOLE = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
          "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
_KEY_ONLY = _WHOLE[:4]


def dino_param_shapes(width, patch, resolution, key_layer):
    """The native executor's parameter table, state-dict name -> shape, in its order: blocks 0 .. key_layer - 1 whole, block
    key_layer with norm1 and qkv only, nothing after it"""
    W, L = width, (resolution // patch) ** 2 + 1
    out = {"cls_token": (1, 1, W), "pos_embed": (1, L, W), "patch_embed.proj.weight": (W, 3, patch, patch), "patch_embed.proj.bias": (W,)}
    block = {"norm1.weight": (W,), "norm1.bias": (W,), "attn.qkv.weight": (3 * W, W), "attn.qkv.bias": (3 * W,), "attn.proj.weight": (W, W),
             "attn.proj.bias": (W,), "norm2.weight": (W,), "norm2.bias": (W,), "mlp.fc1.weight": (4 * W, W), "mlp.fc1.bias": (4 * W,),
             "mlp.fc2.weight": (W, 4 * W), "mlp.fc2.bias": (W,)}
    for i in range(key_layer + 1):
        for k in (_WHOLE if i < key_layer else _KEY_ONLY):
            out[f"blocks.{i}.{k}"] = block[k]
    return out


class DinoNet:
    """Parameters of a DINO ViT up to the keys of block ``key_layer`` under the state-dict names.  A container: there is no
    forward pass."""

    def __init__(self, width=768, layers=12, patch=8, resolution=224, key_layer=None):
        key_layer = layers - 1 if key_layer is None else key_layer
        if width % 64:
            raise ValueError(f"width {width}: the executor needs heads of dimension 64 (width a multiple of 64)")
        if resolution % patch:
            raise ValueError(f"resolution {resolution} is no multiple of the patch size {patch}")
        if not 0 <= key_layer < layers:
            raise ValueError(f"key_layer {key_layer} outside [0, {layers})")
        self.width, self.layers, self.heads, self.patch, self.resolution, self.key_layer = width, layers, width // 64, patch, resolution, key_layer
        self.tokens = (resolution // patch) ** 2 + 1
        self.param_shapes = dino_param_shapes(width, patch, resolution, key_layer)
        self.params = {k: torch.zeros(s) for k, s in self.param_shapes.items()}
        self.ignored = []

    # the scales of init_random: tokens (patch embedding of 0...255 inputs, cls, pos), the attention and MLP branch outputs,
    # and the norm of a key row of block key_layer
    TOKEN_SCALE, ATTN_SCALE, MLP_SCALE, KEY_NORM = 0.02, 0.02, 0.05, 3.4e-3

    def init_random(self, seed=0):
        """Seeded stand-in weights with CHOSEN scales (not N(0, 0.02), under which a wrong GELU or LayerNorm eps barely moves
        the distance): small tokens, so that the LayerNorm eps shows; unit-variance q / k / v; fc1 pre-activations of standard
        deviation 3 and an MLP branch larger than the tokens, so that the form of the GELU shows; key rows of norm about
        3e-3 in block key_layer, so that ``clamp(n_i n_j, 1e-8)`` against ``n_i n_j + 1e-8`` shows (the self-similarity is
        otherwise invariant to the keys' scale)"""
        g = torch.Generator().manual_seed(seed)
        W, p = self.width, self.patch
        ts, key_block = self.TOKEN_SCALE, f"blocks.{self.key_layer}.attn.qkv."
        for name, shape in self.param_shapes.items():
            r = torch.randn(shape, generator=g)
            if name == "patch_embed.proj.weight":
                t = r * (ts / (500.0 * (3 * p * p) ** 0.5))
            elif name in ("cls_token", "pos_embed"):
                t = r * ts
            elif name.endswith("norm1.weight") or name.endswith("norm2.weight"):
                t = 1.0 + 0.1 * r
            elif name.endswith("qkv.weight"):
                t = r / W ** 0.5
            elif name.endswith("fc1.weight"):
                t = r * (3.0 / W ** 0.5)
            elif name.endswith("attn.proj.weight"):
                t = r * (self.ATTN_SCALE * 3 / W ** 0.5)
            elif name.endswith("fc2.weight"):
                t = r * (self.MLP_SCALE / 2 / (4 * W) ** 0.5)
            elif name.endswith("patch_embed.proj.bias") or name.endswith("proj.bias") or name.endswith("fc2.bias"):
                t = r * (0.2 * ts)
            else:                         # norm / qkv / fc1 biases
                t = r * 0.1
            if name.startswith(key_block):
                t[W:2 * W] *= self.KEY_NORM / W ** 0.5
            self.params[name] = t
        return self

    @classmethod
    def from_state_dict(cls, sd, resolution=224, key_layer=11):
        """width / layers / patch from the shapes (heads = width // 64); ``pos_embed`` must hold (resolution / patch)^2 + 1
        rows.  Names the executor does not use (``norm.*``, the blocks after ``key_layer``, the projection and MLP of block
        ``key_layer``, any head) are accepted and listed in ``.ignored``."""
        sd = {re.sub(r"^(module\.|backbone\.)+", "", k): v for k, v in sd.items()}
        for need in ("cls_token", "pos_embed", "patch_embed.proj.weight"):
            if need not in sd:
                raise KeyError(f"state_dict mismatch: {need} is missing (expected a DINO ViT state dict)")
        W = int(sd["cls_token"].shape[-1])
        patch = int(sd["patch_embed.proj.weight"].shape[-1])
        layers = 1 + max([int(m.group(1)) for m in map(_BLOCK.match, sd) if m] or [-1])
        if layers < 1:
            raise KeyError("state_dict mismatch: no blocks.{i}.* entries")
        rows = int(sd["pos_embed"].shape[1])
        if resolution % patch or (resolution // patch) ** 2 + 1 != rows:
            raise ValueError(f"pos_embed has {rows} rows, resolution {resolution} at patch {patch} needs "
                             f"{(resolution // patch) ** 2 + 1 if resolution % patch == 0 else 'a multiple of the patch size'}: "
                             "positional-embedding interpolation is out of scope (pass the resolution the checkpoint was trained at)")
        if rows > MAX_TOKENS:
            raise ValueError(f"{rows} tokens: the executor runs at most {MAX_TOKENS}")
        net = cls(W, layers, patch, resolution, key_layer)
        missing = [k for k in net.param_shapes if k not in sd]
        if missing:
            raise KeyError(f"state_dict mismatch: missing {missing} ({len(missing)})")
        for k, shape in net.param_shapes.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(sd[k].shape)}")
        net.params = {k: sd[k].detach().float() for k in net.param_shapes}
        net.ignored = sorted(k for k in sd if k not in net.param_shapes)
        return net

    def state_dict(self):
        return dict(self.params)


def read_weights(path):
    """A LOCAL torch state-dict file (such as the published ``dino_vitbase8_pretrain.pth``), or a directory holding exactly
    one ``.pth`` -> the dict.  Nothing is fetched."""
    if os.path.isdir(path):
        files = sorted(f for f in os.listdir(path) if f.endswith(".pth"))
        if len(files) != 1:
            raise FileNotFoundError(f"{path}: expected exactly one .pth file, found {len(files)}")
        path = os.path.join(path, files[0])
    elif not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such file or directory (weights are local, nothing is fetched)")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise TypeError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def preprocess_pair(img_pred, img_gt, mask_pred=None, mask_gt=None):
    """matrics_calculator.py:390-406 for one pair: the arrays as float32 in 0...255 (no / 255), ``* mask`` -> two float32
    (3, S, S) tensors.  The resize and the normalisation run on the device (csrc/dino.hip prep_kernel)."""
    a = np.array(img_pred).astype(np.float32)
    b = np.array(img_gt).astype(np.float32)
    if a.shape != b.shape:
        raise ValueError(f"structure distance: image shapes should be the same, got {a.shape} and {b.shape}")
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] != a.shape[1]:
        raise ValueError(f"structure distance: non-square images are out of scope, got an array of shape {a.shape} (expected (S, S, 3))")
    if mask_pred is not None:
        a = a * np.array(mask_pred).astype(np.float32)
    if mask_gt is not None:
        b = b * np.array(mask_gt).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1)))), torch.from_numpy(np.ascontiguousarray(np.transpose(b, (2, 0, 1))))


class NativeDinoStructure(NativeOwner):
    """``weights``: None (seeded stand-in weights of the configuration in ``standin``, synthetic runs), a ``DinoNet``, a state
    dict, or a LOCAL path (``read_weights``).  ``distance`` is bit-identical whatever the batch (``batch_invariant``),
    symmetric in its two arguments, and exactly 0 for equal images."""
    batch_invariant = True
    _family = "dino"

    def __init__(self, weights=None, device="cuda:0", seed=0, resolution=224, key_layer=11, **standin):
        if weights is None:
            self.net = DinoNet(resolution=resolution, **standin).init_random(seed)
        elif isinstance(weights, DinoNet):
            self.net = weights
        else:
            self.net = DinoNet.from_state_dict(weights if isinstance(weights, dict) else read_weights(weights), resolution, key_layer)
        self.device = torch.device(device)
        self.calls = 0                # native distance calls made (tests count them)

    # ------------------------------------------------------------------ the native handle
    def _native(self):
        from . import _lib
        if self._h is not None:
            return self._h
        if self.device.type != "cuda":
            raise RuntimeError("NativeDinoStructure runs on the HIP executor only (there is no CPU path)")
        n = self.net
        return self._native_build(self.device, n.params, _lib.DinoCfg(n.width, n.layers, n.heads, n.patch, n.resolution, n.key_layer))

    def _workspace(self, pairs, S):
        need = self._lib.hedit_dino_workspace_bytes(self._h, pairs, S)
        if need == 0:
            raise ValueError(f"structure distance: {pairs} pair(s) of side {S} are outside what the executor runs")
        return self._grow("_ws", need, self.device)

    def _check(self, t, what):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("NativeDinoStructure runs on the HIP executor only: pass CUDA tensors (there is no CPU path)")
        if t.dim() != 4 or t.shape[1] != 3 or not t.is_floating_point():
            raise ValueError(f"{what}: expected a float (N, 3, S, S) tensor, got {tuple(t.shape)}")
        if t.shape[2] != t.shape[3]:
            raise ValueError(f"{what}: non-square images are out of scope, got {tuple(t.shape)}")
        if t.shape[2] < self.net.patch or t.shape[2] > 4096:
            raise ValueError(f"{what}: side {t.shape[2]} outside [{self.net.patch}, 4096]")

    # ------------------------------------------------------------------ the network and the metric
    def keys(self, images):
        """images: CUDA float (B, 3, S, S), 0...255, already masked -> (B, tokens, width) fp32 keys of block key_layer"""
        from . import _lib
        self._check(images, "keys")
        B, _, S, _ = images.shape
        if B < 1 or B > 2 * MAX_PAIRS:
            raise ValueError(f"keys: batch {B} outside [1, {2 * MAX_PAIRS}]")
        h = self._native()
        x = images.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(B, self.net.tokens, self.net.width, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            ws = self._workspace((B + 1) // 2, S)
            _lib.check(self._lib.hedit_dino_keys(h, _lib.ptr(x), B, S, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.cur_stream()))
        return out

    def _distance_call(self, a, b):
        from . import _lib
        N, _, S, _ = a.shape
        out = torch.empty(N, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            ws = self._workspace(N, S)
            _lib.check(self._lib.hedit_dino_structure_distance(self._h, _lib.ptr(a), _lib.ptr(b), N, S, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                               _lib.cur_stream()))
        self.calls += 1
        return out

    def distance(self, a, b):
        """a, b: CUDA float (N, 3, S, S), 0...255, already masked -> (N,) fp32; one native call per MAX_PAIRS pairs"""
        self._check(a, "distance")
        self._check(b, "distance")
        if a.shape != b.shape:
            raise ValueError(f"distance: expected two tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        if a.shape[0] < 1:
            raise ValueError("distance: an empty batch")
        self._native()
        a = a.detach().to(device=self.device, dtype=torch.float32).contiguous()
        b = b.detach().to(device=self.device, dtype=torch.float32).contiguous()
        return torch.cat([self._distance_call(a[i:i + MAX_PAIRS], b[i:i + MAX_PAIRS]) for i in range(0, a.shape[0], MAX_PAIRS)])

    def scores(self, items):
        """[(img_pred, img_gt[, mask_pred[, mask_gt]]), ...] of one image size -> [float]: the reference's preprocessing per
        pair, then one native call per MAX_PAIRS pairs; by batch invariance the values are those of the ``score`` loop"""
        pairs = [preprocess_pair(*it) for it in items]        # shape errors come first, on the host
        if self.device.type != "cuda":
            raise RuntimeError("NativeDinoStructure runs on the HIP executor only (there is no CPU path)")
        if not pairs:
            return []
        if len({tuple(a.shape) for a, _ in pairs}) != 1:
            raise ValueError("scores: the pairs of one call must have one image size")
        a = torch.stack([p[0] for p in pairs]).to(self.device)
        b = torch.stack([p[1] for p in pairs]).to(self.device)
        return [float(v) for v in self.distance(a, b).cpu()]

    def score(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        return self.scores([(img_pred, img_gt, mask_pred, mask_gt)])[0]
