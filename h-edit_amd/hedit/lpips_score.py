"""SqueezeNet-LPIPS on the native executor (``hedit_sqlpips_*`` of libhedit_hip.so, csrc/sqlpips.hip): the metric the
PIE-Bench evaluator reports in its ``lpips`` / ``lpips_unedit_part`` / ``lpips_edit_part`` columns -- torchmetrics'
``LearnedPerceptualImagePatchSimilarity(net_type='squeeze')`` on ``img * 2 - 1`` of the reference's
text-guided/evaluation/matrics_calculator.py:276,329-347.

The network: ScalingLayer -> torchvision ``squeezenet1_1.features`` with taps after features 1, 4, 7, 9, 10, 11, 12
(64, 128, 256, 384, 384, 512, 512 channels) -> each tap divided by its channel L2 norm (+ 1e-10) -> squared difference ->
non-negative 1x1 ``lin{k}`` weights -> spatial mean -> sum.  PARITY UNPINNED: neither torchmetrics nor lpips nor
torchvision is installed here and the reference tree holds no vector for this metric; what the tests check is the native
executor against a torch restatement of this description (tests/helpers/sqlpips_ref.py).

Nothing is ever fetched: weights come from local files or from seeded stand-in values, and there is no torch forward --
``SqueezeLpipsNet`` is a parameter container, CPU tensors raise.
"""
import os
import re

import numpy as np
import torch

from .native import NativeOwner

# torchvision features index, input channels, squeeze channels, channels of each expand (csrc/sqlpips.hip FIRE)
FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128),
         (9, 256, 48, 192), (10, 384, 48, 192), (11, 384, 64, 256), (12, 512, 64, 256))
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
MAX_BATCH = 64            # HEDIT_SQLPIPS_MAX_BATCH of include/hedit.h
MIN_SIDE = 32


def sqlpips_param_shapes():
    """The native executor's parameter table, canonical name -> shape, in its order"""
    out = {"features.0.weight": (64, 3, 3, 3), "features.0.bias": (64,)}
    for idx, cin, s, e in FIRES:
        p = f"features.{idx}."
        out[p + "squeeze.weight"] = (s, cin, 1, 1)
        out[p + "squeeze.bias"] = (s,)
        out[p + "expand1x1.weight"] = (e, s, 1, 1)
        out[p + "expand1x1.bias"] = (e,)
        out[p + "expand3x3.weight"] = (e, s, 3, 3)
        out[p + "expand3x3.bias"] = (e,)
    for k, c in enumerate(TAP_CHANNELS):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


_SPELLINGS = (re.compile(r"^features\.(\d+)\.(.+)$"),              # torchvision squeezenet1_1
              re.compile(r"^net\.slice\d+\.(\d+)\.(.+)$"),          # the lpips package
              re.compile(r"^net\.slices\.\d+\.(\d+)\.(.+)$"))       # torchmetrics
_IGNORED = ("lins.", "scaling_layer.", "classifier.")


def canonical_names(sd):
    """One state dict in any of three spellings -> canonical names.  The backbone entries are told apart by the torchvision
    index they all carry: ``features.{i}.`` (torchvision ``squeezenet1_1``), ``net.slice{K}.{i}.`` (the lpips package),
    ``net.slices.{K-1}.{i}.`` (torchmetrics).  ``lin{k}.model.1.weight`` is taken as it is; the ``lins.*`` duplicates newer
    lpips versions list, the ``scaling_layer.*`` buffers (compiled into the executor) and torchvision's ``classifier.*`` are
    dropped.  Any other key passes through under its own name, so the strict check of the caller reports it.  These
    spellings come from the published packages; none of them is installed here: NOT VERIFIED AGAINST THE PACKAGES."""
    out = {}
    for k, v in sd.items():
        if k.startswith(_IGNORED):
            continue
        name = k
        for pat in _SPELLINGS:
            m = pat.match(k)
            if m:
                name = f"features.{m.group(1)}.{m.group(2)}"
                break
        if name in out and not torch.equal(torch.as_tensor(out[name]), torch.as_tensor(v)):
            raise KeyError(f"state_dict mismatch: {k} gives {name} a second, different value")
        out[name] = v
    return out


def _read(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise TypeError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def read_weights(weights):
    """A state dict (any spelling), a local file, a local directory holding the backbone file and the lin file (every
    ``.pth`` / ``.pt`` / ``.bin`` in it, in name order), or a pair (backbone, lins) of those -> one dict
    under the canonical names.  Local files only."""
    if isinstance(weights, (tuple, list)):
        parts = [read_weights(w) for w in weights]
    elif isinstance(weights, dict):
        return canonical_names(weights)
    elif os.path.isdir(weights):
        files = sorted(f for f in os.listdir(weights) if f.endswith((".pth", ".pt", ".bin")))
        if not files:
            raise FileNotFoundError(f"{weights}: no .pth / .pt / .bin file (the backbone and the lin weights)")
        parts = [canonical_names(_read(os.path.join(weights, f))) for f in files]
    elif os.path.isfile(weights):
        return canonical_names(_read(weights))
    else:
        raise FileNotFoundError(f"{weights}: no such file or directory (weights are local, nothing is fetched)")
    out = {}
    for p in parts:
        for k, v in p.items():
            if k in out and not torch.equal(torch.as_tensor(out[k]), torch.as_tensor(v)):
                raise KeyError(f"state_dict mismatch: {k} appears twice with different values")
            out[k] = v
    return out


class SqueezeLpipsNet:
    """Parameters of SqueezeNet-LPIPS under the canonical names (``features.{i}...``, ``lin{k}.model.1.weight``).  A
    container: there is no forward pass."""

    def __init__(self):
        self.param_shapes = sqlpips_param_shapes()
        self.params = {k: torch.zeros(s) for k, s in self.param_shapes.items()}

    def init_random(self, seed=0):
        """Seeded stand-in weights: He-scaled convolutions, small biases, non-negative lin weights (as the trained ones)"""
        g = torch.Generator().manual_seed(seed)
        for name, shape in self.param_shapes.items():
            if name.startswith("lin"):
                t = torch.rand(shape, generator=g) / shape[1]
            elif len(shape) > 1:
                t = torch.randn(shape, generator=g) * (2.0 / float(np.prod(shape[1:]))) ** 0.5
            else:
                t = 0.05 * torch.randn(shape, generator=g)
            self.params[name] = t
        return self

    def load_state_dict(self, sd):
        """Strict: after ``canonical_names`` exactly the table's names, with the table's shapes"""
        sd = canonical_names(sd)
        missing = [k for k in self.param_shapes if k not in sd]
        extra = [k for k in sd if k not in self.param_shapes]
        if missing or extra:
            raise KeyError(f"state_dict mismatch: missing {missing} ({len(missing)}), unexpected {extra} ({len(extra)})")
        for k, shape in self.param_shapes.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(sd[k].shape)}")
        self.params = {k: sd[k].detach().float() for k in self.param_shapes}
        return self

    def state_dict(self):
        return dict(self.params)


def preprocess_pair(img_pred, img_gt, mask_pred=None, mask_gt=None):
    """matrics_calculator.py:329-344 for one pair: ``array / 255`` as float32, ``* mask``, ``* 2 - 1`` -> two float32
    (3, H, W) tensors in [-1, 1]"""
    a = np.array(img_pred).astype(np.float32) / 255
    b = np.array(img_gt).astype(np.float32) / 255
    assert a.shape == b.shape, "Image shapes should be the same."
    if mask_pred is not None:
        a = a * np.array(mask_pred).astype(np.float32)
    if mask_gt is not None:
        b = b * np.array(mask_gt).astype(np.float32)
    return (torch.tensor(a).permute(2, 0, 1) * 2 - 1).contiguous(), (torch.tensor(b).permute(2, 0, 1) * 2 - 1).contiguous()


class NativeSqueezeLpips(NativeOwner):
    """``weights``: None (seeded stand-in weights, synthetic runs), a local path, a state dict, or a pair (backbone, lins)
    of those -- see ``read_weights``.  ``distance`` is bit-identical whatever the batch (``batch_invariant``), symmetric in
    its two arguments, and exactly 0 for equal images."""
    batch_invariant = True
    _family = "sqlpips"

    def __init__(self, weights=None, device="cuda:0", seed=0):
        self.net = SqueezeLpipsNet()
        if weights is None:
            self.net.init_random(seed)
        else:
            self.net.load_state_dict(read_weights(weights))
        self.device = torch.device(device)
        self.calls = 0                # native distance calls made (tests count them)

    # ------------------------------------------------------------------ the native handle
    def _native(self):
        if self._h is not None:
            return self._h
        if self.device.type != "cuda":
            raise RuntimeError("NativeSqueezeLpips runs on the HIP executor only (there is no CPU / torch path)")
        return self._native_build(self.device, self.net.params)

    # ------------------------------------------------------------------ the metric
    def distance(self, a, b):
        """a, b: CUDA float (N, 3, H, W) tensors in [-1, 1] -> (N,) fp32, LPIPS(a_n, b_n); ONE native call"""
        from . import _lib
        for t in (a, b):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("NativeSqueezeLpips runs on the HIP executor only: pass CUDA tensors (there is no CPU / torch path)")
        if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape or not a.is_floating_point() or not b.is_floating_point():
            raise ValueError(f"distance: expected two float (N, 3, H, W) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        N, _, H, W = a.shape
        if N < 1 or N > MAX_BATCH:
            raise ValueError(f"distance: batch {N} outside [1, {MAX_BATCH}]")
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"distance: images of {H} x {W}, the network needs at least {MIN_SIDE} x {MIN_SIDE}")
        h = self._native()
        dev = self.device
        a = a.detach().to(device=dev, dtype=torch.float32).contiguous()
        b = b.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty(N, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            need = self._lib.hedit_sqlpips_workspace_bytes(h, N, H, W)
            self._grow("_ws", max(need, 1), dev)
            _lib.check(self._lib.hedit_sqlpips_distance(h, _lib.ptr(a), _lib.ptr(b), N, H, W, _lib.ptr(out), _lib.ptr(self._ws), self._ws.numel(),
                                                        _lib.cur_stream()))
        self.calls += 1
        return out

    def scores(self, items):
        """[(img_pred, img_gt[, mask_pred[, mask_gt]]), ...] of one image size -> [float]: the reference's preprocessing per
        pair, then ONE native call per MAX_BATCH pairs; by batch invariance the values are those of the ``score`` loop"""
        if self.device.type != "cuda":
            raise RuntimeError("NativeSqueezeLpips runs on the HIP executor only (there is no CPU / torch path)")
        pairs = [preprocess_pair(*it) for it in items]
        if not pairs:
            return []
        if len({tuple(a.shape) for a, _ in pairs}) != 1:
            raise ValueError("scores: the pairs of one call must have one image size")
        out = []
        for i in range(0, len(pairs), MAX_BATCH):
            chunk = pairs[i:i + MAX_BATCH]
            a = torch.stack([p[0] for p in chunk]).to(self.device)
            b = torch.stack([p[1] for p in chunk]).to(self.device)
            out += [float(v) for v in self.distance(a, b).cpu()]
        return out

    def score(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        return self.scores([(img_pred, img_gt, mask_pred, mask_gt)])[0]
