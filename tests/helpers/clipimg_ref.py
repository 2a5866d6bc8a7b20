"""Test infrastructure for the native CLIP image tower (csrc/clipimg.hip on csrc/encoder.hip / encoder.h, hedit.clip_score): hash-seeded weights under the
OpenAI CLIP names (what tests/golden/make_golden_clipimg.py loaded into the reference's CLIP and into transformers'
CLIPModel, regenerated identically by the tests -- on the device for the ViT-L/14 shape), the name mapping to
transformers' layout, and a plain restatement of the tower in torch.  Nothing here is product code."""
import numpy as np
import torch
import torch.nn.functional as F

from .text_ref import name_seed

# the sizes of tests/golden/g20_clipimg.*: a toy tower at 17 tokens (56 px) and at 257 tokens (224 px), patch 14, sharing
# the embedding space of helpers.text_ref.TOY's text tower (proj_dim 32), and the ViT-L/14 vision shape
TOY17 = dict(width=128, layers=3, heads=2, patch_size=14, input_resolution=56, embed_dim=32)
TOY257 = dict(TOY17, input_resolution=224)
L14 = dict(width=1024, layers=24, heads=16, patch_size=14, input_resolution=224, embed_dim=768)


def _hash_uniform_t(n, seed, device):
    """helpers.tiny.hash_uniform in torch (any device), bit for bit: the same 64-bit integer mix in wrapping int64
    arithmetic, logical right shifts emulated by masking the sign extension"""
    def lsr(x, k):
        return (x >> k) & ((1 << (64 - k)) - 1)

    def i64(v):
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >= (1 << 63) else v

    x = torch.arange(n, dtype=torch.int64, device=device) + i64(seed * 0x9E3779B97F4A7C15)
    x = x ^ lsr(x, 30)
    x = x * i64(0xBF58476D1CE4E5B9)
    x = x ^ lsr(x, 27)
    x = x * i64(0x94D049BB133111EB)
    x = x ^ lsr(x, 31)
    return lsr(x, 40).to(torch.float32) / float(1 << 24)


def hash_normal_t(shape, seed, device="cpu"):
    """helpers.tiny.hash_normal in torch (any device), bit for bit"""
    n = int(np.prod(shape))
    u = 0.0 + _hash_uniform_t(n, seed * 4, device)
    for i in range(1, 4):
        u = u + _hash_uniform_t(n, seed * 4 + i, device)
    return ((u - 2.0) * float(np.float32(np.sqrt(3.0)))).reshape(shape)


def clipimg_weights(width, layers, patch_size, input_resolution, embed_dim, device="cpu", **unused):
    """name -> fp32 tensor, OpenAI CLIP names; every tensor a function of its name and shape alone (elementwise fp32
    arithmetic only, so the device does not change a bit)."""
    from hedit.clip_score import clipimg_param_shapes
    out = {}
    for name, shape in clipimg_param_shapes(width, layers, patch_size, input_resolution, embed_dim).items():
        v = hash_normal_t(shape, name_seed(name), device)
        if name.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight")):
            v = 1.0 + 0.1 * v
        elif name in ("visual.class_embedding", "visual.positional_embedding", "visual.proj"):
            v = v * float(np.float32(float(width) ** -0.5))
        elif len(shape) == 1:
            v = 0.1 * v
        else:
            v = v * float(np.float32(float(np.prod(shape[1:])) ** -0.5))
        out[name] = v.float().contiguous()
    return out


def clip_to_hf_vision(sd):
    """OpenAI CLIP image-tower names -> transformers CLIPModel names (in_proj split into q, k, v in that order)."""
    top = {"visual.class_embedding": "vision_model.embeddings.class_embedding", "visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
           "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
           "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
           "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias"}
    ren = (("ln_1", "layer_norm1"), ("attn.out_proj", "self_attn.out_proj"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
           ("mlp.c_proj", "mlp.fc2"))
    out = {}
    for k, v in sd.items():
        if k in top:
            out[top[k]] = v
        elif k == "visual.proj":
            out["visual_projection.weight"] = v.t().contiguous()
        else:
            i, rest = k[len("visual.transformer.resblocks."):].split(".", 1)
            dst = f"vision_model.encoder.layers.{i}."
            if rest.startswith("attn.in_proj_"):
                s = rest[len("attn.in_proj_"):]
                for name, part in zip("qkv", v.chunk(3, dim=0)):
                    out[f"{dst}self_attn.{name}_proj.{s}"] = part.contiguous()
                continue
            for a, b in ren:
                if rest.startswith(a + "."):
                    out[dst + b + rest[len(a):]] = v
                    break
            else:
                raise KeyError(k)
    return out


def test_images(n, resolution, seed, device="cpu"):
    """n CLIP-normalised-looking images [n][3][R][R], a function of (n, R, seed) alone"""
    return hash_normal_t((n, 3, resolution, resolution), seed, device).float().contiguous()


def image_forward(sd, images, heads, dtype=torch.float32):
    """(B, embed_dim): patch embedding, class token + positions, ln_pre, pre-LN blocks with bidirectional attention and
    QuickGELU, ln_post on the class row, times visual.proj."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    W = p["visual.class_embedding"].shape[0]
    patch = p["visual.conv1.weight"].shape[-1]
    x = F.conv2d(images.to(dtype), p["visual.conv1.weight"], stride=patch)
    B = x.shape[0]
    x = x.reshape(B, W, -1).permute(0, 2, 1)
    x = torch.cat([p["visual.class_embedding"].expand(B, 1, W), x], dim=1) + p["visual.positional_embedding"]
    x = F.layer_norm(x, (W,), p["visual.ln_pre.weight"], p["visual.ln_pre.bias"])
    L, hd = x.shape[1], W // heads
    i = 0
    while f"visual.transformer.resblocks.{i}.ln_1.weight" in p:
        g = lambda s: p[f"visual.transformer.resblocks.{i}.{s}"]      # noqa: E731
        y = F.layer_norm(x, (W,), g("ln_1.weight"), g("ln_1.bias"))
        q, k, v = F.linear(y, g("attn.in_proj_weight"), g("attn.in_proj_bias")).chunk(3, dim=-1)
        q, k, v = (t.reshape(B, L, heads, hd).transpose(1, 2) for t in (q, k, v))
        a = ((q * hd ** -0.5) @ k.transpose(-1, -2)).softmax(-1)
        o = (a @ v).transpose(1, 2).reshape(B, L, W)
        x = x + F.linear(o, g("attn.out_proj.weight"), g("attn.out_proj.bias"))
        y = F.layer_norm(x, (W,), g("ln_2.weight"), g("ln_2.bias"))
        y = F.linear(y, g("mlp.c_fc.weight"), g("mlp.c_fc.bias"))
        x = x + F.linear(y * torch.sigmoid(1.702 * y), g("mlp.c_proj.weight"), g("mlp.c_proj.bias"))
        i += 1
    x = F.layer_norm(x[:, 0], (W,), p["visual.ln_post.weight"], p["visual.ln_post.bias"])
    return x @ p["visual.proj"]


def cosines(img, txt):
    """[n_img][n_txt] cosines in float64"""
    a, b = img.double(), txt.double()
    return (a / a.norm(dim=-1, keepdim=True)) @ (b / b.norm(dim=-1, keepdim=True)).t()


def uint8_image(h, w, seed):
    """a reproducible uint8 (h, w, 3) image: smooth ramps plus hash noise, so that the bicubic resize has something to do"""
    from .tiny import hash_uniform
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([xx / w, yy / h, (xx + yy) / (w + h)], -1)
    noise = hash_uniform((h, w, 3), seed).numpy()
    return np.clip((0.6 * base + 0.4 * noise) * 255.0, 0, 255).astype(np.uint8)
