#!/usr/bin/env python3
"""PIE-Bench evaluation driver -- the CLI, dataset handling and CSV format of the reference's
text-guided/evaluation/evaluation.py (:9-25 run-length mask decoding, :27-92 metric dispatch, :103-215 main) for the
outputs of h-edit_amd/main_p2p.py.

Metrics.  The pixel metrics are computed here with the formulas of the torchmetrics classes the reference
instantiates (evaluation/matrics_calculator.py:272-279): ``psnr`` (PeakSignalNoiseRatio(data_range=1)), ``mse``
(MeanSquaredError), ``ssim`` (StructuralSimilarityIndexMeasure(data_range=1): 11 x 11 Gaussian window, sigma 1.5,
k1 0.01, k2 0.03, reflect padding, mean over the interior), each on the whole image / the edited part / the unedited
part exactly as the reference masks them (image * mask before the metric).

``clip_similarity_source_image`` / ``_target_image`` / ``_target_image_edit_part`` (torchmetrics CLIPScore on CLIP ViT-L/14,
matrics_calculator.py:274,290-302) run on the native CLIP towers (hedit/clip_score.py, csrc/clipimg.hip + csrc/text.hip)
when a LOCAL model is given with ``--clip_path`` (a transformers-style directory, or an OpenAI ``.pt`` together with
``--clip_tokenizer DIR``) and ``--device cuda``; nothing is ever fetched.  ``lpips`` / ``lpips_unedit_part`` /
``lpips_edit_part`` (torchmetrics LPIPS with net_type='squeeze' on ``img * 2 - 1``, matrics_calculator.py:276,329-347) run
on the native SqueezeNet-LPIPS (hedit/lpips_score.py, csrc/sqlpips.hip) when LOCAL weights are given with ``--lpips_path``
(one state-dict file, or a directory holding the backbone file and the lin file) and ``--device cuda``.
``structure_distance`` / ``structure_distance_unedit_part`` / ``structure_distance_edit_part`` (the mean squared difference
of the DINO ViT-B/8 key self-similarity matrices, matrics_calculator.py:12-246,390-410) run on the native DINO key
extractor (hedit/dino_score.py, csrc/dino.hip) when a LOCAL state dict is given with ``--dino_path`` (the published
``dino_vitbase8_pretrain.pth``, or a directory holding exactly one ``.pth``) and ``--device cuda``.  ``local_clip`` (the CLIP
directional similarity of local_clip_evaluation.py as matrics_calculator.py:304-307,320-321 runs it: ViT-L/14, the direction
term alone, masks ignored) runs on the same towers plus the native image preprocessing and direction head
(hedit/local_clip_score.py, csrc/imgprep.hip) when ``--clip_path`` and ``--local_clip_templates FILE`` are given: the prompt
templates are the user's input, one per line with one ``{}`` each -- none is shipped.  Asking for a network metric without
its model raises with the name of what is missing instead of writing a made-up number.

``--native_preprocess`` (with ``--clip_path`` and ``--device cuda``) moves the image preprocessing of the clip_similarity_*
columns to the device (hedit/image_prep.py): PIL's bicubic resample bit for bit, so the CSV does not change by a byte.

``--native_pixel`` (with ``--device cuda``) moves the pixel columns themselves to the native executor (hedit/pixel_score.py,
csrc/pixmetrics.hip): the same formulas on the uint8 images, fp64 after the fp32 difference, binary masks only.  ``--batch N``
evaluates up to N (annotation entry, method) pairs of one image size per scorer call -- every native scorer is bit-identical
whatever the batch, so the CSV is byte for byte the ``--batch 1`` one.
"""
import argparse
import csv
import json
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

PIXEL_METRICS = ("psnr", "mse", "ssim")
PIXEL_METRICS_ORDER = ("mse", "psnr", "ssim")        # the columns of a pixel scorer's 3 x 3 result (hedit.pixel_score.METRICS)
NETWORK_METRICS = {"lpips": "torchmetrics LPIPS (SqueezeNet) weights", "structure_distance": "DINO ViT-B/8 weights (a local state dict: --dino_path)",
                   "clip_similarity_source_image": "CLIP ViT-L/14 weights", "clip_similarity_target_image": "CLIP ViT-L/14 weights",
                   "clip_similarity_target_image_edit_part": "CLIP ViT-L/14 weights", "local_clip": "a local CLIP ViT-L/14 model (--clip_path) and a prompt-template file (--local_clip_templates)"}


try:
    from hedit.pie_mask import mask_decode  # noqa: F401  (the run-length mask decoding, shared with main_masactrl.py)
except ImportError:      # run as a script: the `hedit` package lies one directory up
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hedit.pie_mask import mask_decode  # noqa: F401


def _pair(img_pred, img_gt, mask_pred, mask_gt, scale=255.0):
    a = np.array(img_pred).astype(np.float32) / scale
    b = np.array(img_gt).astype(np.float32) / scale
    assert a.shape == b.shape, "Image shapes should be the same."
    if mask_pred is not None:
        a = a * np.array(mask_pred).astype(np.float32)
    if mask_gt is not None:
        b = b * np.array(mask_gt).astype(np.float32)
    return torch.tensor(a).permute(2, 0, 1)[None], torch.tensor(b).permute(2, 0, 1)[None]


def _gauss(size=11, sigma=1.5):
    d = torch.arange((1 - size) / 2, (1 + size) / 2, dtype=torch.float32)
    g = torch.exp(-(d / sigma) ** 2 / 2)
    g = g / g.sum()
    return (g[:, None] @ g[None, :])


def _require_cuda(device, what, who="the CLIP towers run"):
    """the network metrics have no CPU execution path: say so instead of failing somewhere inside the library"""
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{what} on device {str(device)!r}: {who} on the HIP executor only (there is no CPU path); "
                           "use --device cuda")


class MetricsCalculator:
    """The pixel metrics and the CLIP score of the reference's MetricsCalculator (matrics_calculator.py:271-390), same method
    names.  `clip`: a CLIP scorer (hedit.clip_score.NativeClip); without one ``calculate_clip_similarity`` raises.  `lpips`:
    an LPIPS scorer (hedit.lpips_score.NativeSqueezeLpips); without one ``calculate_lpips`` raises.  `dino`: a structure
    scorer (hedit.dino_score.NativeDinoStructure); without one ``calculate_structure_distance`` raises.  `pixel`: a pixel
    scorer (hedit.pixel_score.NativePixelMetrics); without one ``calculate_mse`` / ``_psnr`` / ``_ssim`` are the torch code below.
    `local_clip`: a directional-similarity scorer (hedit.local_clip_score.NativeLocalClip); without one ``compute_local_clip`` raises."""

    def __init__(self, device="cpu", clip=None, lpips=None, dino=None, pixel=None, local_clip=None):
        self.device = device
        self.clip = clip              # hedit.clip_score.NativeClip (or anything with score(uint8 H x W x 3 array, text)), or None
        self.lpips = lpips            # hedit.lpips_score.NativeSqueezeLpips (or anything with score(pred, gt, mask_pred, mask_gt)), or None
        if clip is not None:
            _require_cuda(device, "CLIP score")
        self.dino = dino              # hedit.dino_score.NativeDinoStructure (or anything with score(pred, gt, mask_pred, mask_gt)), or None
        if lpips is not None:
            _require_cuda(device, "LPIPS", "SqueezeNet-LPIPS runs")
        if dino is not None:
            _require_cuda(device, "structure distance", "the DINO key extractor runs")
        self.pixel = pixel            # hedit.pixel_score.NativePixelMetrics (or anything with score(metric, pred, gt, mask_pred, mask_gt)), or None
        if pixel is not None:
            _require_cuda(device, "native pixel metrics", "the pixel-metrics kernel runs")
        self.local_clip = local_clip  # hedit.local_clip_score.NativeLocalClip (or anything with score(src, src prompt, tgt, tgt prompt)), or None
        if local_clip is not None:
            _require_cuda(device, "local_clip")

    def compute_local_clip(self, src_img, src_prompt, tar_img, tar_prompt, mask=None):
        """matrics_calculator.py:304-327: the directional similarity of the two images and the two prompts; the reference
        takes a mask and never uses it (its CLIPLoss runs the direction term alone), so it is ignored here too"""
        if self.local_clip is None:
            raise NotImplementedError("local_clip: needs " + NETWORK_METRICS["local_clip"] + ", which this run does not have")
        return float(self.local_clip.score(src_img, src_prompt, tar_img, tar_prompt))

    def calculate_structure_distance(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        """matrics_calculator.py:390-410: both images as float32 in 0...255 (NOT / 255), times their masks, through the DINO
        key self-similarity (the scorer does that preprocessing: the resize and the normalisation go with the network)"""
        if self.dino is None:
            raise NotImplementedError("structure_distance: needs " + NETWORK_METRICS["structure_distance"] + ", which this run does not have")
        assert np.array(img_pred).shape == np.array(img_gt).shape, "Image shapes should be the same."
        return float(self.dino.score(img_pred, img_gt, mask_pred, mask_gt))

    def calculate_lpips(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        """matrics_calculator.py:329-347: both images / 255, times their masks, * 2 - 1, through SqueezeNet-LPIPS (the
        scorer does that preprocessing: it goes with the network's input convention)"""
        if self.lpips is None:
            raise NotImplementedError("lpips: needs " + NETWORK_METRICS["lpips"] + " (local files: --lpips_path), which this run does not have")
        assert np.array(img_pred).shape == np.array(img_gt).shape, "Image shapes should be the same."
        return float(self.lpips.score(img_pred, img_gt, mask_pred, mask_gt))

    def calculate_clip_similarity(self, img, txt, mask=None):
        """matrics_calculator.py:290-302: the image (times the mask, back to uint8) and the prompt through CLIPScore"""
        if self.clip is None:
            raise NotImplementedError("clip similarity: needs " + NETWORK_METRICS["clip_similarity_target_image"] +
                                      " (a local model: --clip_path), which this run does not have")
        img = np.array(img)
        if mask is not None:
            mask = np.array(mask)
            img = np.uint8(img * mask)
        return float(self.clip.score(img, txt))

    def calculate_mse(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        if self.pixel is not None:
            return float(self.pixel.score("mse", img_pred, img_gt, mask_pred, mask_gt))
        a, b = _pair(img_pred, img_gt, mask_pred, mask_gt)
        return float(((a.to(self.device) - b.to(self.device)) ** 2).mean().item())

    def calculate_psnr(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        if self.pixel is not None:
            return float(self.pixel.score("psnr", img_pred, img_gt, mask_pred, mask_gt))
        a, b = _pair(img_pred, img_gt, mask_pred, mask_gt)
        mse = ((a.to(self.device) - b.to(self.device)) ** 2).mean()
        return float((10.0 * torch.log10(1.0 / mse)).item())                 # data_range = 1

    def calculate_ssim(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        if self.pixel is not None:
            return float(self.pixel.score("ssim", img_pred, img_gt, mask_pred, mask_gt))
        a, b = _pair(img_pred, img_gt, mask_pred, mask_gt)
        a, b = a.to(self.device), b.to(self.device)
        C = a.shape[1]
        k = _gauss().to(self.device)[None, None].expand(C, 1, 11, 11).contiguous()
        pad = 5
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        ap, bp = F.pad(a, (pad,) * 4, mode="reflect"), F.pad(b, (pad,) * 4, mode="reflect")
        stack = torch.cat([ap, bp, ap * ap, bp * bp, ap * bp])
        out = F.conv2d(stack, k, groups=C)
        mu_a, mu_b, saa, sbb, sab = out.split(1)
        va, vb, vab = saa - mu_a ** 2, sbb - mu_b ** 2, sab - mu_a * mu_b
        ssim = ((2 * mu_a * mu_b + c1) * (2 * vab + c2)) / ((mu_a ** 2 + mu_b ** 2 + c1) * (va + vb + c2))
        return float(ssim[..., pad:-pad, pad:-pad].mean().item())             # torchmetrics crops the padded border again


def calculate_metric(mc, metric, src_image, tgt_image, src_mask, tgt_mask, src_prompt, tgt_prompt):
    base = metric
    part = None
    for suffix in ("_unedit_part", "_edit_part"):
        if metric.endswith(suffix) and not metric.startswith("clip_similarity"):
            base, part = metric[:-len(suffix)], suffix
    if metric.startswith("clip_similarity_") and metric in NETWORK_METRICS and getattr(mc, "clip", None) is not None:
        if metric == "clip_similarity_source_image":
            return mc.calculate_clip_similarity(src_image, src_prompt, None)
        if metric == "clip_similarity_target_image":
            return mc.calculate_clip_similarity(tgt_image, tgt_prompt, None)
        if tgt_mask.sum() == 0:
            return "nan"
        return mc.calculate_clip_similarity(tgt_image, tgt_prompt, tgt_mask)
    if metric == "local_clip" and getattr(mc, "local_clip", None) is not None:
        return mc.compute_local_clip(src_image, src_prompt, tgt_image, tgt_prompt)
    routed = PIXEL_METRICS + (("lpips",) if getattr(mc, "lpips", None) is not None else ()) + \
        (("structure_distance",) if getattr(mc, "dino", None) is not None else ())
    if (base in NETWORK_METRICS or metric in NETWORK_METRICS) and base not in routed:
        raise NotImplementedError(f"metric {metric}: needs {NETWORK_METRICS.get(base, NETWORK_METRICS.get(metric))}, which this offline "
                                  "build does not have; pixel metrics: " + ", ".join(PIXEL_METRICS))
    if base not in routed:
        raise ValueError(f"unknown metric {metric}")
    fn = getattr(mc, "calculate_" + base)
    if part is None:
        return fn(src_image, tgt_image, None, None)
    if part == "_unedit_part":
        if (1 - src_mask).sum() == 0 or (1 - tgt_mask).sum() == 0:
            return "nan"
        return fn(src_image, tgt_image, 1 - src_mask, 1 - tgt_mask)
    if src_mask.sum() == 0 or tgt_mask.sum() == 0:
        return "nan"
    return fn(src_image, tgt_image, src_mask, tgt_mask)


def _split_metric(metric):
    """(base, part) as calculate_metric splits a column name; part is None, "_unedit_part" or "_edit_part" """
    for suffix in ("_unedit_part", "_edit_part"):
        if metric.endswith(suffix) and not metric.startswith("clip_similarity"):
            return metric[:-len(suffix)], suffix
    return metric, None


def _grouped_request(mc, metric, it):
    """What calculate_metric would hand to a scorer for column `metric` of item `it` (a dict with src, tgt, mask, src_p,
    tgt_p): "nan" where one of its nan rules fires, (family, arguments) for a scorer call, or None for everything that is not
    a scorer call (the torch pixel path, a refusal): calculate_metric itself then runs for that item."""
    src, tgt, mask = it["src"], it["tgt"], it["mask"]
    if metric.startswith("clip_similarity_") and metric in NETWORK_METRICS and getattr(mc, "clip", None) is not None:
        if metric == "clip_similarity_source_image":
            return "clip", (np.array(src), it["src_p"])
        if metric == "clip_similarity_target_image":
            return "clip", (np.array(tgt), it["tgt_p"])
        if mask.sum() == 0:
            return "nan"
        return "clip", (np.uint8(np.array(tgt) * np.array(mask)), it["tgt_p"])
    if metric == "local_clip" and getattr(mc, "local_clip", None) is not None:
        return "local_clip", (src, it["src_p"], tgt, it["tgt_p"])
    base, part = _split_metric(metric)
    family = {"lpips": "lpips", "structure_distance": "dino"}.get(base, "pixel" if base in PIXEL_METRICS else None)
    if family is None or getattr(mc, family, None) is None:
        return None
    if part is None:
        return family, (src, tgt, None, None)
    if part == "_unedit_part":
        if (1 - mask).sum() == 0:
            return "nan"
        return family, (src, tgt, 1 - mask, 1 - mask)
    if mask.sum() == 0:
        return "nan"
    return family, (src, tgt, mask, mask)


def evaluate_group(mc, metrics, items):
    """Every column of `metrics` for every item of the group (one image size) -> one list of values per item, the values
    calculate_metric gives item by item.  A scorer with a batched ``scores`` gets one call per column -- the pixel scorer ONE
    call for all its columns: an item's whole / edit / unedit parts come out of the same native call --, a scorer without one
    is called item by item.  The nan rules are applied per item before anything reaches a scorer."""
    values = [[None] * len(metrics) for _ in items]
    requests = [[_grouped_request(mc, m, it) for m in metrics] for it in items]
    pixel_rows = {}
    pixel = getattr(mc, "pixel", None)
    if pixel is not None and hasattr(pixel, "scores"):
        live = [i for i, reqs in enumerate(requests) if any(isinstance(r, tuple) and r[0] == "pixel" for r in reqs)]
        if live:
            def item(i):
                masked = any(isinstance(r, tuple) and r[0] == "pixel" and r[1][2] is not None for r in requests[i])
                it = items[i]
                return (it["src"], it["tgt"], it["mask"], it["mask"]) if masked else (it["src"], it["tgt"])
            pixel_rows = dict(zip(live, pixel.scores([item(i) for i in live])))
    for j, metric in enumerate(metrics):
        base, part = _split_metric(metric)
        calls = []
        for i, it in enumerate(items):
            r = requests[i][j]
            if r == "nan":
                values[i][j] = "nan"
            elif r is None or (r[0] == "pixel" and i not in pixel_rows):
                values[i][j] = calculate_metric(mc, metric, it["src"], it["tgt"], it["mask"], it["mask"], it["src_p"], it["tgt_p"])
            elif r[0] == "pixel":
                values[i][j] = float(pixel_rows[i][(None, "_edit_part", "_unedit_part").index(part), PIXEL_METRICS_ORDER.index(base)])
            else:
                calls.append((i, r))
        if not calls:
            continue
        family = calls[0][1][0]
        scorer = getattr(mc, family)
        if family not in ("clip", "local_clip"):
            for _, (_, a) in calls:
                assert np.array(a[0]).shape == np.array(a[1]).shape, "Image shapes should be the same."
        if hasattr(scorer, "scores"):
            got = scorer.scores([a[0] for _, (_, a) in calls], [a[1] for _, (_, a) in calls]) if family == "clip" else \
                scorer.scores([a for _, (_, a) in calls])
        else:
            got = [scorer.score(*a) for _, (_, a) in calls]
        for (i, _), v in zip(calls, got):
            values[i][j] = float(v)
    return values


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--annotation_mapping_file', type=str, default="./PIE_Bench_Data/mapping_file.json")
    p.add_argument('--metrics', nargs='+', type=str, default=["psnr_unedit_part", "mse_unedit_part", "ssim_unedit_part"])
    p.add_argument('--src_image_folder', type=str, default="./PIE_Bench_Data/annotation_images")
    p.add_argument('--tgt_methods', nargs='+', type=str, default=["your_method"])
    p.add_argument('--tgt_folders', nargs='+', type=str, default=None,
                   help="one result directory per entry of --tgt_methods (the reference hard-codes this table in the script)")
    p.add_argument('--result_path', type=str, default="./results/results.csv")
    p.add_argument('--device', type=str, default="cpu")
    p.add_argument('--edit_category_list', nargs='+', type=str, default=[str(i) for i in range(10)])
    p.add_argument('--clip_path', type=str, default=None,
                   help="LOCAL CLIP model for the clip_similarity_* metrics: an openai/clip-vit-large-patch14-style directory "
                        "(config.json, weights, tokenizer files) or an OpenAI .pt file (then also --clip_tokenizer)")
    p.add_argument('--clip_tokenizer', type=str, default=None, help="local directory with the CLIP tokenizer files, for a bare .pt --clip_path")
    p.add_argument('--lpips_path', type=str, default=None,
                   help="LOCAL SqueezeNet-LPIPS weights for the lpips* metrics: one state-dict file (lpips / torchmetrics spelling), or a "
                        "directory holding the backbone file (torchvision squeezenet1_1) and the lin file")
    p.add_argument('--dino_path', type=str, default=None,
                   help="LOCAL DINO ViT state dict for the structure_distance* metrics: the published dino_vitbase8_pretrain.pth, or a "
                        "directory holding exactly one .pth")
    p.add_argument('--dino_resolution', type=int, default=224,
                   help="the side the DINO input is resized to; the checkpoint's pos_embed must fit it (no interpolation)")
    p.add_argument('--local_clip_templates', type=str, default=None,
                   help="prompt templates of the local_clip metric (needs --clip_path): a UTF-8 file, one template per line with one "
                        "'{}' each; blank lines and lines starting with # are skipped")
    p.add_argument('--native_preprocess', action="store_true",
                   help="preprocess the images of the clip_similarity_* columns on the device (needs --device cuda and --clip_path); "
                        "the CSV is byte for byte the same")
    p.add_argument('--native_pixel', action="store_true",
                   help="compute the psnr* / mse* / ssim* columns with the native pixel-metrics kernel (needs --device cuda; binary masks)")
    p.add_argument('--batch', type=int, default=1,
                   help="evaluate up to N (annotation entry, method) pairs of one image size per scorer call; the CSV is byte for byte "
                        "the --batch 1 one")
    return p


def load_clip(clip_path, clip_tokenizer, device):
    """The native CLIP of --clip_path on `device` (local files only)"""
    _require_cuda(device, "--clip_path")
    from hedit.clip_score import NativeClip
    dev = "cuda:0" if str(device) == "cuda" else device
    if os.path.isdir(clip_path):
        return NativeClip.from_pretrained(clip_path, device=dev)
    if not clip_tokenizer:
        raise SystemExit("--clip_path is a file (an OpenAI CLIP .pt): give --clip_tokenizer DIR with the tokenizer files")
    return NativeClip.from_openai_checkpoint(clip_path, clip_tokenizer, device=dev)


def load_lpips(lpips_path, device):
    """The native SqueezeNet-LPIPS of --lpips_path on `device` (local files only)"""
    _require_cuda(device, "--lpips_path", "SqueezeNet-LPIPS runs")
    from hedit.lpips_score import NativeSqueezeLpips
    return NativeSqueezeLpips(lpips_path, device="cuda:0" if str(device) == "cuda" else device)


def load_dino(dino_path, device, resolution=224):
    """The native DINO structure scorer of --dino_path on `device` (a local file only; torch.hub is never called)"""
    _require_cuda(device, "--dino_path", "the DINO key extractor runs")
    from hedit.dino_score import NativeDinoStructure
    return NativeDinoStructure(dino_path, device="cuda:0" if str(device) == "cuda" else device, resolution=resolution)


def load_pixel(device):
    """The native pixel-metrics scorer of --native_pixel on `device`"""
    _require_cuda(device, "--native_pixel", "the pixel-metrics kernel runs")
    from hedit.pixel_score import NativePixelMetrics
    return NativePixelMetrics(device="cuda:0" if str(device) == "cuda" else device)


def load_local_clip(clip, templates_path):
    """The native local_clip scorer on the towers of --clip_path with the templates of --local_clip_templates"""
    from hedit.local_clip_score import NativeLocalClip, load_templates
    return NativeLocalClip(clip, load_templates(templates_path))


def _entries(args, folders, annotation):
    """(key, source image, mask, source prompt, target prompt, [target image per method]) per selected annotation entry, read
    exactly as the per-image loop of main reads them"""
    for key, item in annotation.items():
        if item["editing_type_id"] not in args.edit_category_list:
            continue
        src_image = Image.open(os.path.join(args.src_image_folder, item["image_path"])).convert("RGB")
        mask = mask_decode(item.get("mask", []), image_shape=(src_image.size[1], src_image.size[0]))
        mask = mask[:, :, np.newaxis].repeat([3], axis=2)
        src_p = item["original_prompt"].replace("[", "").replace("]", "")
        tgt_p = item["editing_prompt"].replace("[", "").replace("]", "")
        tgts = []
        for folder in folders.values():
            tgt = Image.open(os.path.join(folder, item["image_path"])).convert("RGB")
            if tgt.size[0] != tgt.size[1]:       # result sheets: the edited image is the right-most square (evaluation.py:203-205)
                s = src_image.size[0]
                tgt = tgt.crop((tgt.size[0] - s, tgt.size[1] - s, tgt.size[0], tgt.size[1]))
            tgts.append(tgt)
        yield key, src_image, mask, src_p, tgt_p, tgts


def _run_grouped(args, mc, folders, entries):
    """--batch N > 1: the (annotation entry, method) pairs in annotation order, in groups of up to N of one image size; a row
    is written as soon as it and every row before it are complete"""
    pending, group, written = [], [], 0          # pending: [key, values per (method, metric)] in annotation order

    def flush():
        nonlocal written
        if group:
            for it, vals in zip(group, evaluate_group(mc, args.metrics, group)):
                it["row"][it["at"]:it["at"] + len(vals)] = vals
            group.clear()
        while pending and all(v is not None for v in pending[0]):
            with open(args.result_path, 'a+', newline="") as f:
                csv.writer(f).writerow(pending.pop(0))
            written += 1

    for key, src_image, mask, src_p, tgt_p, tgts in entries:
        row = [key] + [None] * (len(folders) * len(args.metrics))
        pending.append(row)
        for k, tgt in enumerate(tgts):
            it = dict(src=src_image, tgt=tgt, mask=mask, src_p=src_p, tgt_p=tgt_p, row=row, at=1 + k * len(args.metrics))
            if group and (group[0]["src"].size, group[0]["tgt"].size) != (src_image.size, tgt.size):
                flush()
            group.append(it)
            if len(group) >= args.batch:
                flush()
    flush()
    return written


def main(argv=None, clip=None, lpips=None, dino=None, pixel=None, local_clip=None):
    """`clip` / `lpips` / `dino` / `pixel` / `local_clip`: ready scorers instead of --clip_path / --lpips_path / --dino_path /
    --native_pixel / --local_clip_templates (synthetic runs and tests: NativeClip.from_standin, NativeSqueezeLpips(),
    NativeDinoStructure(), NativePixelMetrics(), NativeLocalClip(clip, templates))"""
    args = build_parser().parse_args(argv)
    if args.batch < 1:
        raise SystemExit("--batch N: N >= 1")
    if not args.tgt_folders or len(args.tgt_folders) != len(args.tgt_methods):
        raise SystemExit("give --tgt_folders DIR ... (one per method)")
    folders = dict(zip(args.tgt_methods, args.tgt_folders))
    if args.local_clip_templates and local_clip is None and clip is None and not args.clip_path:
        raise SystemExit("--local_clip_templates FILE needs the CLIP towers: give --clip_path too")
    if args.native_preprocess:
        _require_cuda(args.device, "--native_preprocess", "the image-preprocessing kernel runs")
        if clip is None and not args.clip_path:
            raise SystemExit("--native_preprocess preprocesses the images of the CLIP columns: give --clip_path too")
    if clip is None and args.clip_path:
        clip = load_clip(args.clip_path, args.clip_tokenizer, args.device)
    if args.native_preprocess:
        clip.native_preprocess = True
    if local_clip is None and args.local_clip_templates:
        local_clip = load_local_clip(clip, args.local_clip_templates)
    if lpips is None and args.lpips_path:
        lpips = load_lpips(args.lpips_path, args.device)
    if dino is None and args.dino_path:
        dino = load_dino(args.dino_path, args.device, args.dino_resolution)
    if pixel is None and args.native_pixel:
        pixel = load_pixel(args.device)
    mc = MetricsCalculator(args.device, clip, lpips, dino, pixel=pixel, local_clip=local_clip)
    os.makedirs(os.path.dirname(os.path.abspath(args.result_path)), exist_ok=True)
    with open(args.result_path, 'w', newline="") as f:
        csv.writer(f).writerow(["file_id"] + [f"{k}|{m}" for k in folders for m in args.metrics])
    with open(args.annotation_mapping_file) as f:
        annotation = json.load(f)
    if args.batch > 1:
        rows = _run_grouped(args, mc, folders, _entries(args, folders, annotation))
        print(f"evaluated {rows} image(s) -> {args.result_path}")
        return rows
    rows = 0
    for key, item in annotation.items():
        if item["editing_type_id"] not in args.edit_category_list:
            continue
        src_image = Image.open(os.path.join(args.src_image_folder, item["image_path"])).convert("RGB")
        mask = mask_decode(item.get("mask", []), image_shape=(src_image.size[1], src_image.size[0]))
        mask = mask[:, :, np.newaxis].repeat([3], axis=2)
        src_p = item["original_prompt"].replace("[", "").replace("]", "")
        tgt_p = item["editing_prompt"].replace("[", "").replace("]", "")
        row = [key]
        for name, folder in folders.items():
            tgt = Image.open(os.path.join(folder, item["image_path"])).convert("RGB")
            if tgt.size[0] != tgt.size[1]:       # result sheets: the edited image is the right-most square (evaluation.py:203-205)
                s = src_image.size[0]
                tgt = tgt.crop((tgt.size[0] - s, tgt.size[1] - s, tgt.size[0], tgt.size[1]))
            for metric in args.metrics:
                row.append(calculate_metric(mc, metric, src_image, tgt, mask, mask, src_p, tgt_p))
        with open(args.result_path, 'a+', newline="") as f:
            csv.writer(f).writerow(row)
        rows += 1
    print(f"evaluated {rows} image(s) -> {args.result_path}")
    return rows


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the `hedit` package, for the native scorers
    main()
