"""What the Prompt-to-Prompt generation / attention-viewer tests share: a seeded fake attention store for the hook path, the
fp64 restatement of aggregate_attention (reference text-guided/p2p/ptp_classes.py:298-309) and of hedit_attn_aggregate's
definition (include/hedit.h), and their error bounds."""
import numpy as np
import torch

HEADS = 2
STEPS = 3
# (place, is_cross, tokens) of the fake UNet's attention layers, in call order: 8 x 8 and 4 x 4 token layers
LAYERS = [("down", True, 64), ("down", False, 64), ("down", True, 16), ("down", False, 16),
          ("mid", True, 16), ("mid", False, 16),
          ("up", True, 16), ("up", False, 16), ("up", True, 64), ("up", False, 64), ("up", True, 64), ("up", False, 64)]
U = 2.0 ** -24          # unit roundoff of fp32


def fake_steps(seed=0):
    """STEPS x len(LAYERS) tensors (2 prompts * HEADS, tokens, 77 | tokens) in [0, 1): what a controller's forward() is handed
    as the conditional half of each layer"""
    g = torch.Generator().manual_seed(seed)
    return [[torch.rand(2 * HEADS, tok, 77 if is_cross else tok, generator=g) for _, is_cross, tok in LAYERS] for _ in range(STEPS)]


def fill_store(store, steps):
    """the steps through store.forward / between_steps, as AttentionControl.__call__ drives them on the hook path (the store
    accumulates INTO the first step's tensors, so it is handed clones)"""
    for step in steps:
        for (place, is_cross, _), attn in zip(LAYERS, step):
            store.forward(attn.clone(), is_cross, place, True)
        store.cur_step += 1
        store.between_steps()
    return store


def aggregate_ref64(steps, res, from_where, is_cross, select):
    """fp64: the mean over the selected layers and heads of (sum over steps) / STEPS -> (value (res,res,K), sum of |terms|, count)"""
    terms = []
    for location in from_where:
        for li, (place, cross, tok) in enumerate(LAYERS):
            if place == location and cross == is_cross and tok == res * res:
                acc = sum(step[li].double() for step in steps) / len(steps)
                terms += list(acc.reshape(2, HEADS, res, res, acc.shape[-1])[select])
    if not terms:
        return None, None, 0
    t = torch.stack(terms)
    return t.sum(0) / len(terms), t.abs().sum(0), len(terms)


def hook_path_bound(abs_sum, count):
    """|fp32 composition - fp64| per element.  Each term carries STEPS - 1 rounded additions and one division
    (<= STEPS * U relative); torch sums the `count` terms in some order (<= (count - 1) * U * sum|t|, the bound of any
    summation order) and divides once more: (count + STEPS) * U * sum|t| / count to first order, one more U for the rest."""
    return (count + STEPS + 1) * U * abs_sum / count


def kernel_ref64(maps, cur_step):
    """hedit_attn_aggregate's definition in fp64.  maps: list of (n_img, 2, heads, tokens, cols) tensors.
    -> (value (n_img, 2, tokens, cols), bound): terms acc / cur_step, their mean; the elementwise bound
    (n_maps * heads + 2) * 2^-24 * sum|terms| / (n_maps * heads) of a left-to-right fp32 sum plus the two divisions."""
    terms = torch.cat([m.double() / cur_step for m in maps], dim=2)        # (n_img, 2, n_maps * heads, tokens, cols)
    count = terms.shape[2]
    return terms.sum(2) / count, (count + 2) * U * terms.abs().sum(2) / count


def torch_aggregate(avg_maps, res, from_where, is_cross, select, n_prompts=2):
    """the reference's composition over a get_average_attention() dict, on whatever device its tensors live"""
    out = [item.reshape(n_prompts, -1, res, res, item.shape[-1])[select] for location in from_where
           for item in avg_maps[f"{location}_{'cross' if is_cross else 'self'}"] if item.shape[1] == res * res]
    out = torch.cat(out, dim=0)
    return out.sum(0) / out.shape[0]


class StubTokenizer:
    """encode / decode of a whitespace vocabulary with CLIP's start and end tokens"""

    def __init__(self):
        self.words = ["<s>", "</s>"]

    def encode(self, text):
        ids = []
        for w in text.split():
            if w not in self.words:
                self.words.append(w)
            ids.append(self.words.index(w))
        return [0] + ids + [1]

    def decode(self, i):
        return self.words[int(i)]


def as_numpy(t):
    return np.asarray(t.detach().cpu())
