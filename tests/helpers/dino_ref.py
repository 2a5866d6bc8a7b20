"""The Structure Distance restated in torch on the CPU (fp64 by default), written from the public DINO ViT architecture
(facebookresearch/dino vision_transformer.py) and the five steps of hedit/dino_score.py's docstring -- the reference the
native executor (csrc/dino.hip on csrc/encoder.hip / encoder.h) is tested against.  Every wrong variant the tests must be able to see is a switch here:
``gelu`` (erf / tanh / quick), ``eps``, ``div255``, ``antialias``, ``key_layer``, ``clamp``.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# the parity cases of tests/test_gpu_dino.py: name -> (width, layers, key_layer, patch, R, S, weight seed)
CASES = {
    "t26": (128, 3, 2, 8, 40, 64, 21),        # 26 tokens: one ragged key tile, every Gram tile ragged
    "t145": (128, 3, 2, 8, 96, 128, 22),      # 145 tokens: crosses key-tile boundaries, ragged tail
    "t785": (128, 3, 2, 8, 224, 512, 23),     # 785 tokens: production's tile counts and resize ratio
    "p16": (384, 3, 2, 16, 224, 224, 24),     # 197 tokens, no resize, patch 16
    "vitb": (768, 3, 2, 8, 224, 512, 25),     # production GEMM shapes
}


def uint8_pair(S, seed):
    """two related S x S x 3 uint8 images: smooth structure plus noise, the second a perturbed copy"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / S
    base = np.stack([0.5 + 0.4 * np.sin(2 * math.pi * (f * xx + (c + 1) * yy) + c) for c, f in enumerate((1.0, 2.0, 3.0))], -1)
    a = np.clip(base + 0.15 * g.standard_normal((S, S, 3)), 0, 1)
    b = np.clip(a + 0.2 * np.sin(2 * math.pi * 3 * xx)[..., None] + 0.1 * g.standard_normal((S, S, 3)), 0, 1)
    return (a * 255).astype(np.uint8), (b * 255).astype(np.uint8)


def upper_half_mask(S):
    m = np.zeros((S, S, 3), np.float64)
    m[: S // 2] = 1
    return m


def resize(x, R):
    """(B, 3, S, S) -> (B, 3, R, R): bilinear, align_corners=False, no antialias, written out (not F.interpolate):
    src = (dst + 0.5) S / R - 0.5 clamped at 0, the upper neighbour clamped to S - 1.  S == R is the identity."""
    S = x.shape[-1]
    if S == R:
        return x
    src = ((torch.arange(R, dtype=x.dtype) + 0.5) * (S / R) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=S - 1)
    i1 = (i0 + 1).clamp(max=S - 1)
    l1 = src - i0.to(x.dtype)
    l0 = 1 - l1
    rows = x[:, :, i0, :] * l0[:, None] + x[:, :, i1, :] * l1[:, None]
    return rows[:, :, :, i0] * l0 + rows[:, :, :, i1] * l1


def preprocess(x, R, div255=False, antialias=False):
    """x (B, 3, S, S) in 0...255 -> resized and normalised AS THE REFERENCE DOES: the ImageNet constants on 0...255 values"""
    if div255:
        x = x / 255
    x = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False, antialias=True) if antialias and x.shape[-1] != R else resize(x, R)
    mean = torch.tensor(MEAN, dtype=x.dtype)[None, :, None, None]
    std = torch.tensor(STD, dtype=x.dtype)[None, :, None, None]
    return (x - mean) / std


def _gelu(t, kind):
    if kind == "erf":
        return 0.5 * t * (1 + torch.erf(t * (0.5 ** 0.5)))
    if kind == "tanh":
        return 0.5 * t * (1 + torch.tanh(math.sqrt(2 / math.pi) * (t + 0.044715 * t ** 3)))
    if kind == "quick":
        return t * torch.sigmoid(1.702 * t)
    raise ValueError(kind)


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def tokens(params, img, patch):
    """normalised image (B, 3, R, R) -> the token stream entering block 0, (B, L, W)"""
    P = {k: v for k, v in params.items()}
    x = F.conv2d(img, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=patch)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([P["cls_token"].expand(x.shape[0], -1, -1), x], 1)
    return x + P["pos_embed"]


def keys_from_tokens(params, x, key_layer, gelu="erf", eps=1e-6):
    """blocks 0 .. key_layer - 1 whole, then norm1 and the key third of qkv of block key_layer: (B, L, W)"""
    W = x.shape[-1]
    heads = W // 64
    for i in range(key_layer):
        p = f"blocks.{i}."
        B, L, _ = x.shape
        qkv = _ln(x, params[p + "norm1.weight"], params[p + "norm1.bias"], eps) @ params[p + "attn.qkv.weight"].T + params[p + "attn.qkv.bias"]
        q, k, v = qkv.reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
        att = torch.softmax((q @ k.transpose(-2, -1)) * 64 ** -0.5, -1)
        o = (att @ v).transpose(1, 2).reshape(B, L, W)
        x = x + o @ params[p + "attn.proj.weight"].T + params[p + "attn.proj.bias"]
        hdn = _ln(x, params[p + "norm2.weight"], params[p + "norm2.bias"], eps) @ params[p + "mlp.fc1.weight"].T + params[p + "mlp.fc1.bias"]
        x = x + _gelu(hdn, gelu) @ params[p + "mlp.fc2.weight"].T + params[p + "mlp.fc2.bias"]
    p = f"blocks.{key_layer}."
    return _ln(x, params[p + "norm1.weight"], params[p + "norm1.bias"], eps) @ params[p + "attn.qkv.weight"][W:2 * W].T + params[p + "attn.qkv.bias"][W:2 * W]


def keys(params, x, patch, R, key_layer, dtype=torch.float64, gelu="erf", eps=1e-6, div255=False, antialias=False):
    """x (B, 3, S, S) in 0...255, masked -> the keys (B, L, W) in `dtype`"""
    P = {k: v.to(dtype) for k, v in params.items()}
    with torch.no_grad():
        return keys_from_tokens(P, tokens(P, preprocess(x.to(dtype), R, div255, antialias), patch), key_layer, gelu, eps)


def self_sim(K, clamp=True):
    n = K.norm(dim=-1, keepdim=True)
    f = n @ n.transpose(-2, -1)
    return (K @ K.transpose(-2, -1)) / (f.clamp(min=1e-8) if clamp else f + 1e-8)


def distance(params, a, b, patch, R, key_layer, dtype=torch.float64, clamp=True, **variant):
    """a, b (N, 3, S, S) in 0...255, masked -> (N,) tensor of mean((S_a - S_b)^2) in `dtype`"""
    ka = keys(params, a, patch, R, key_layer, dtype, **variant)
    kb = keys(params, b, patch, R, key_layer, dtype, **variant)
    return ((self_sim(ka, clamp) - self_sim(kb, clamp)) ** 2).mean((-2, -1))


# ---- the limits of tests/test_gpu_dino.py (derivation and the measured figures: that file's docstring)
LIM = 4e-5          # |native - ref| <= LIM |ref| + 1e-9 for a distance: 16 x 2.0e-6, rounded up to one digit
KEY_LIM = 7e-5      # max|native - ref| <= KEY_LIM max|ref| for keys: 16 x 3.8e-6, rounded up to one digit


def parity_inputs(name):
    """the two pairs of a parity case, whole and with the upper half masked: (a, b), float32 (2, 3, S, S) in 0...255"""
    S, seed = CASES[name][5], CASES[name][6]
    a8, b8 = uint8_pair(S, 100 + seed)
    m = upper_half_mask(S).astype(np.float32)
    a, b = a8.astype(np.float32), b8.astype(np.float32)
    chw = lambda x: torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))      # noqa: E731
    return torch.stack([chw(a), chw(a * m)]), torch.stack([chw(b), chw(b * m)])


def net_of(name):
    """the stand-in network of a parity case (hedit.dino_score.DinoNet with its chosen scales)"""
    from hedit.dino_score import DinoNet
    W, layers, k, patch, R, _, seed = CASES[name]
    return DinoNet(W, layers, patch, R, k).init_random(seed)
