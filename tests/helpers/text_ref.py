"""Test infrastructure for the native prompt encoder (csrc/text.hip on csrc/encoder.hip / encoder.h, hedit.text.NativeClipText): hash-seeded weights
under the OpenAI CLIP names (what tests/golden/make_golden_text.py loaded into the reference's CLIP and into transformers'
CLIPTextModel, regenerated identically by the tests), the name mapping to transformers' layout, and a plain restatement
of the text transformer in torch.  Nothing here is product code."""
import zlib

import torch
import torch.nn.functional as F

from .tiny import hash_normal, hash_uniform

# the sizes of tests/golden/g19_text.*: a toy tower (reference CLIP and transformers) and one at SD-1.x width with a
# reduced vocabulary
TOY = dict(width=128, layers=3, heads=2, vocab_size=512, context_length=77, proj_dim=32)
SDW = dict(width=768, layers=12, heads=12, vocab_size=1024, context_length=77, proj_dim=0)


def name_seed(name):
    return zlib.crc32(name.encode()) % 100003


def text_weights(width, layers, vocab_size, context_length, proj_dim=0, heads=None):
    """name -> fp32 tensor, OpenAI CLIP names; every tensor a function of its name and shape alone."""
    from hedit.text import text_param_shapes
    out = {}
    for name, shape in text_param_shapes(width, layers, vocab_size, context_length, proj_dim).items():
        v = hash_normal(shape, name_seed(name))
        if name == "token_embedding.weight":
            v = 0.02 * v
        elif name == "positional_embedding":
            v = 0.01 * v
        elif name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):
            v = 1.0 + 0.1 * v
        elif len(shape) == 1:
            v = 0.1 * v
        elif name == "text_projection":
            v = v * float(shape[0]) ** -0.5
        else:
            v = v * float(shape[1]) ** -0.5
        out[name] = v.float().contiguous()
    return out


def clip_to_hf(sd, prefix=""):
    """OpenAI CLIP text-tower names -> transformers CLIPTextModel names (in_proj split into q, k, v in that order)."""
    out = {}
    ren = (("ln_1", "layer_norm1"), ("attn.out_proj", "self_attn.out_proj"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
           ("mlp.c_proj", "mlp.fc2"))
    for k, v in sd.items():
        if k == "token_embedding.weight":
            out[prefix + "embeddings.token_embedding.weight"] = v
        elif k == "positional_embedding":
            out[prefix + "embeddings.position_embedding.weight"] = v
        elif k.startswith("ln_final."):
            out[prefix + "final_layer_norm." + k.split(".")[1]] = v
        elif k == "text_projection":
            out[prefix + "text_projection.weight"] = v.t().contiguous()
        else:
            _, _, i, rest = k.split(".", 3)
            dst = f"{prefix}encoder.layers.{i}."
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


def word_ids(n, seed, lo, hi, exclude=()):
    """n reproducible token ids in [lo, hi) that avoid `exclude`"""
    u = hash_uniform((4 * n + 8,), seed).numpy()
    out = [i for i in (lo + int(x * (hi - lo)) for x in u) if i not in exclude][:n]
    assert len(out) == n
    return out


def text_forward(sd, ids, heads, eos_token_id=None, dtype=torch.float32):
    """(hidden (B, L, W) after ln_final, pooled): pre-LN blocks, causal attention, QuickGELU, the pooled row at
    ids.argmax(-1) or at the first `eos_token_id`, times text_projection when `sd` has one."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    W = p["ln_final.weight"].shape[0]
    B, L = ids.shape
    hd = W // heads
    x = p["token_embedding.weight"][ids] + p["positional_embedding"][:L][None]
    mask = torch.full((L, L), float("-inf"), dtype=dtype).triu(1)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in p:
        g = lambda s: p[f"transformer.resblocks.{i}.{s}"]      # noqa: E731
        y = F.layer_norm(x, (W,), g("ln_1.weight"), g("ln_1.bias"))
        q, k, v = F.linear(y, g("attn.in_proj_weight"), g("attn.in_proj_bias")).chunk(3, dim=-1)
        q, k, v = (t.reshape(B, L, heads, hd).transpose(1, 2) for t in (q, k, v))
        a = ((q * hd ** -0.5) @ k.transpose(-1, -2) + mask).softmax(-1)
        o = (a @ v).transpose(1, 2).reshape(B, L, W)
        x = x + F.linear(o, g("attn.out_proj.weight"), g("attn.out_proj.bias"))
        y = F.layer_norm(x, (W,), g("ln_2.weight"), g("ln_2.bias"))
        y = F.linear(y, g("mlp.c_fc.weight"), g("mlp.c_fc.bias"))
        x = x + F.linear(y * torch.sigmoid(1.702 * y), g("mlp.c_proj.weight"), g("mlp.c_proj.bias"))
        i += 1
    h = F.layer_norm(x, (W,), p["ln_final.weight"], p["ln_final.bias"])
    pos = ids.argmax(-1) if eos_token_id is None else (ids == eos_token_id).int().argmax(-1)
    pooled = h[torch.arange(B), pos]
    if "text_projection" in p:
        pooled = pooled @ p["text_projection"]
    return h, pooled


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())
