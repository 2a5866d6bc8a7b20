"""Test infrastructure for hedit.local_clip_score: the direction head restated in torch float64, a tiny stand-in CLIP (hash-seeded
weights under the OpenAI names, image tower 64 wide / 3 layers / patch 4 / 16 px = 17 tokens, text tower 64 wide / 2 layers, the
word tokenizer), and the whole metric in float64 from tests/helpers/clipimg_ref.py::image_forward, text_ref.py::text_forward,
PIL preprocessing (imgprep_ref.torchvision_ref) and the formulas.  Nothing here is product code."""
import functools

import torch

from . import clipimg_ref as CR
from . import imgprep_ref as IR
from . import text_ref as TR

IMG = dict(width=64, layers=3, heads=1, patch_size=4, input_resolution=16, embed_dim=32)
TXT = dict(width=64, layers=2, heads=1, vocab_size=49408, context_length=77, proj_dim=32)
TEMPLATES = ["a photo of a {}.", "a sketch of the {}.", "{} in the rain."]
PROMPTS = ("a brown cat sitting on a wooden bench", "one white dog running through the tall grass today")
SEEDS = (41, 42)          # two independent 40 x 56 images
DELTA = 1e-4              # the towers' parity limit (relative L2 of an embedding against fp64), tests/test_gpu_clip_score.py
LIMIT_CEILING = 0.05


def direction_ref(txt, img):
    """(P, 2, T, E), (P, 2, E) -> float64 (P,): the formulas of hedit/local_clip_score.py in torch float64"""
    txt, img = txt.double(), img.double()
    n = txt / txt.norm(dim=-1, keepdim=True)
    d = (n[:, 1] - n[:, 0]).mean(dim=1)
    D = d / d.norm(dim=-1, keepdim=True)
    u = img / img.norm(dim=-1, keepdim=True)
    e = u[:, 1] - u[:, 0]
    eh = e / (e.norm(dim=-1, keepdim=True) + 1e-7)
    return torch.nn.functional.cosine_similarity(eh, D, dim=-1, eps=1e-8)


@functools.lru_cache(maxsize=None)
def weights():
    """(image-tower state dict, text-tower state dict), a function of the names and shapes alone"""
    return (CR.clipimg_weights(**IMG),
            TR.text_weights(TXT["width"], TXT["layers"], TXT["vocab_size"], TXT["context_length"], TXT["proj_dim"]))


def tokenizer():
    from hedit.text import WordTokenizer
    return WordTokenizer(stable_ids=True)


def images():
    return [IR.image(56, 40, s) for s in SEEDS]


def token_ids(tok, prompts):
    L, eos = TXT["context_length"], tok.eos_token_id
    rows = []
    for p in prompts:
        ids = tok.encode(p)
        assert len(ids) <= L
        rows.append(ids + [eos] * (L - len(ids)))
    return torch.tensor(rows, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def reference():
    """The metric of (images()[0], PROMPTS[0], images()[1], PROMPTS[1]) in float64 -> dict(value, norm_e, norm_d, limit).
    limit = 8 DELTA (1 / |b^ - a^| + 1 / |d|): normalising moves a vector by at most 2 DELTA, a difference of two such by at
    most 4 DELTA, normalising the difference doubles its relative error, and the cosine of two unit vectors moves by at most
    the sum of their movements."""
    wi, wt = weights()
    tok = tokenizer()
    with torch.no_grad():
        x = torch.stack([IR.torchvision_ref(a, IMG["input_resolution"]) for a in images()])
        img = CR.image_forward(wi, x, IMG["heads"], torch.float64)
        full = [t.format(p) for p in PROMPTS for t in TEMPLATES]
        txt = TR.text_forward(wt, token_ids(tok, full), TXT["heads"], tok.eos_token_id, torch.float64)[1]
    txt = txt.reshape(1, 2, len(TEMPLATES), -1)
    value = float(direction_ref(txt, img[None])[0])
    n = txt / txt.norm(dim=-1, keepdim=True)
    nd = float((n[0, 1] - n[0, 0]).mean(dim=0).norm())
    u = img / img.norm(dim=-1, keepdim=True)
    ne = float((u[1] - u[0]).norm())
    return dict(value=value, norm_e=ne, norm_d=nd, limit=8 * DELTA * (1 / ne + 1 / nd))
