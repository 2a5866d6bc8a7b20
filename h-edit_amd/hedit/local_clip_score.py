"""The ``local_clip`` column of the PIE-Bench evaluator on the native executors: the CLIP directional similarity of the
reference's text-guided/evaluation/local_clip_evaluation.py as matrics_calculator.py:304-307,320-321 runs it --
``CLIPLoss(device)`` with its defaults, so ``lambda_direction = 1``, every other term 0, ViT-L/14, the ``DirectionMetric``.

For one (source image, source prompt, target image, target prompt) and templates ``tpl_0 .. tpl_{T-1}``:

  s_j = encode_text(tpl_j.format(source prompt)), t_j likewise for the target prompt, each normalised per template
  d = mean_j (t^_j - s^_j),  D = d / |d|
  a, b = encode_image of the preprocessed source / target image, each normalised
  e = b^ - a^,  e^ = e / (|e| + 1e-7);  the value is cos(e^, D) (torch's CosineSimilarity, eps 1e-8).  Masks are ignored.

Images go through the torchvision convention of hedit/image_prep.py (PIL bilinear to 224, rounding centre crop, fp32 / 255,
CLIP mean and std) on the device, both towers are those of a ``NativeClip``, the head is ``hedit_clip_direction``
(csrc/imgprep.hip), fp64 after the fp32 loads.  Every stage is bit-identical whatever the batch, so ``scores`` gives the values
of the ``score`` loop.

Differences from the reference, all on purpose: its towers run in fp16 on the GPU, ours keep an fp32 stream; a prompt longer
than the context is cut as ``NativeClip.tokenize`` cuts it where ``clip.tokenize`` raises; the RN50 its constructor also loads
is not built, because nothing evaluates it.  The prompt templates are an input: the reference's list is program text of the
reference and is not shipped -- ``load_templates`` reads the user's file.
"""
import torch

from .image_prep import NativeImagePrep

MAX_PAIRS = 64            # HEDIT_CLIP_DIRECTION_MAX_PAIRS of include/hedit.h
MAX_TEMPLATES = 256       # HEDIT_CLIP_DIRECTION_MAX_TEMPLATES
TEXT_CHUNK = 256          # prompts per text-tower call
_NO_CPU = "NativeLocalClip runs on the HIP executor only (there is no CPU path)"


def _check_template(t, where):
    if not isinstance(t, str) or t.count("{}") != 1 or t.replace("{}", "").count("{") or t.replace("{}", "").count("}"):
        raise ValueError(f"{where}: a template has exactly one '{{}}' (and no other brace), got {t!r}")
    return t


def load_templates(path):
    """UTF-8, one template per line, each with exactly one ``{}``; blank lines and lines starting with ``#`` are skipped"""
    out = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            out.append(_check_template(line, f"{path}:{n}"))
    if not out:
        raise ValueError(f"{path}: no templates")
    return out


def direction(txt, img):
    """txt: CUDA float32 (P, 2, T, E), img: CUDA float32 (P, 2, E) -> CUDA float64 (P,): ONE ``hedit_clip_direction`` launch"""
    from . import _lib
    if not (torch.is_tensor(txt) and torch.is_tensor(img) and txt.is_cuda and img.is_cuda):
        raise RuntimeError(_NO_CPU + ": pass CUDA tensors")
    if txt.dim() != 4 or img.dim() != 3 or txt.shape[1] != 2 or tuple(img.shape) != (txt.shape[0], 2, txt.shape[3]) or \
            txt.dtype != torch.float32 or img.dtype != torch.float32:
        raise ValueError(f"direction: expected float32 (P, 2, T, E) and (P, 2, E), got {tuple(txt.shape)} and {tuple(img.shape)}")
    P, _, T, E = txt.shape
    txt, img = txt.contiguous(), img.contiguous()
    out = torch.empty(P, device=txt.device, dtype=torch.float64)
    with torch.cuda.device(txt.device):
        _lib.check(_lib.lib().hedit_clip_direction(_lib.ptr(txt), _lib.ptr(img), P, T, E, _lib.ptr(out), _lib.cur_stream()))
    return out


class NativeLocalClip:
    """``NativeLocalClip(clip, templates)``: `clip` a ``hedit.clip_score.NativeClip``, `templates` a list of strings with one
    ``{}`` each (``load_templates``)."""
    load_templates = staticmethod(load_templates)

    def __init__(self, clip, templates):
        self.clip = clip
        self.templates = [_check_template(t, "templates") for t in templates]
        if not 1 <= len(self.templates) <= MAX_TEMPLATES:
            raise ValueError(f"{len(self.templates)} templates: the head takes 1 to {MAX_TEMPLATES}")
        self.prep = None
        self.calls = 0                # head launches made (tests count them)

    def _text(self, prompts):
        """{prompt: (T, E) features} for the distinct prompts, the T x distinct template prompts in chunks of TEXT_CHUNK"""
        full = [t.format(p) for p in prompts for t in self.templates]
        feats = torch.cat([self.clip.text_features(full[i:i + TEXT_CHUNK]) for i in range(0, len(full), TEXT_CHUNK)])
        T = len(self.templates)
        return {p: feats[i * T:(i + 1) * T] for i, p in enumerate(prompts)}

    def _images(self, images):
        dev = self.clip.image.device
        if dev.type != "cuda":
            raise RuntimeError(_NO_CPU)
        if self.prep is None or self.prep.device != dev:
            self.prep = NativeImagePrep(dev)
        return self.clip.image(self.prep(images, self.clip.image.input_resolution, "torchvision"))

    def scores(self, items):
        """[(src_img, src_prompt, tgt_img, tgt_prompt), ...] of one image size -> [float]: each distinct prompt is encoded
        once, all images go through one preprocessing call and one image-tower call, then one head launch (per MAX_PAIRS
        items).  Bit for bit the values of the ``score`` loop."""
        items = [tuple(it) for it in items]
        out = []
        for i in range(0, len(items), MAX_PAIRS):
            chunk = items[i:i + MAX_PAIRS]
            distinct = list(dict.fromkeys(p for it in chunk for p in (it[1], it[3])))
            text = self._text(distinct)
            img = self._images([im for it in chunk for im in (it[0], it[2])])
            txt = torch.stack([torch.stack([text[it[1]], text[it[3]]]) for it in chunk])
            got = direction(txt, img.reshape(len(chunk), 2, -1))
            self.calls += 1
            out.extend(float(v) for v in got.cpu())
        return out

    def score(self, src_img, src_prompt, tgt_img, tgt_prompt):
        return self.scores([(src_img, src_prompt, tgt_img, tgt_prompt)])[0]
