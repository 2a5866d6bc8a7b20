#!/usr/bin/env python3
"""Generate tests/golden/g17_face_parsing.{npz,json} by RUNNING THE REFERENCE's face-parsing network and mask.

Runs only where the reference tree is present.  It imports the reference's ``FaceParsing``
(face-swapping/arcface/face_parsing_model.py), ``encode_segmentation`` and ``SoftErosion`` (arcface/face_utils.py)
UNMODIFIED, loads the hash-seeded weights of tests/helpers/parsing.py and evaluates, per case, exactly what
main_edit.py:184-191 does with one source image: labels of the model in its default (training) mode, called one image
at a time, then encode_segmentation -> face + mouth -> SoftErosion(13, 0.9, 7).  Also stored: the labels of the model in
eval mode (running statistics); the top-1 - top-2 logit margin of both, read from the classifier's output by a forward
hook and clipped at MARGIN_CLIP; the field SoftErosion thresholds (its last conv2d output, recorded through a wrapper of
the module's ``F``), kept where it lies within FIELD_BAND of the threshold (elsewhere soft / hard imply it); and the
reference's parameter table.  Outputs are data only (inputs + expected outputs).

    python tests/golden/make_golden_parsing.py
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/face-swapping"
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers.parsing import parsing_state_dict  # noqa: E402

THRESH, KSIZE, ITERS = 0.9, 13, 7
MARGIN_CLIP, FIELD_BAND = 1e-3, 1e-3


def synthetic_rgb(h, w, seed):
    """deterministic smooth-ish uint8 image from integer arithmetic (stored in the fixture as it is)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    ch = [((x * (3 + c) + y * (5 - c) + seed * 17) % 256 + ((x * y + c * 31) // 7) % 64) % 256 for c in range(3)]
    return np.stack(ch, -1).astype(np.uint8)


def demo_face(name):
    from PIL import Image
    img = Image.open(os.path.join(REF, "assets", "demo", name)).convert("RGB").resize((256, 256), Image.BILINEAR)
    return np.asarray(img, dtype=np.uint8).copy()


def to_tensor(rgb):
    """uint8 HWC -> [-1, 1] (1, 3, H, W), as main_edit.py:160-163 (ToTensor, * 2 - 1)"""
    return (torch.from_numpy(rgb).permute(2, 0, 1).float().div(255) * 2 - 1).unsqueeze(0)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; the fixture can only be (re)generated where it is")
    sys.path.insert(0, REF)
    from arcface.face_parsing_model import FaceParsing
    import arcface.face_utils as fu

    torch.manual_seed(0)
    probe = FaceParsing()
    table = [[k, list(v.shape)] for k, v in probe.state_dict().items()]
    sd = parsing_state_dict({k: tuple(s) for k, s in table})
    train = FaceParsing()
    train.load_state_dict(sd)           # strict; never .eval(): BatchNorm uses the batch's statistics, as in main_edit.py
    evalm = FaceParsing()
    evalm.load_state_dict(copy.deepcopy(sd))
    evalm.eval()

    logits = {}

    def hook(_m, _i, out):
        logits["last"] = out.detach().clone()
    train.final.register_forward_hook(hook)
    evalm.final.register_forward_hook(hook)

    # SoftErosion's thresholded field = its last conv2d output: record it through a wrapper of the module's F
    rec = {}

    def conv2d(*a, **k):
        y = F.conv2d(*a, **k)
        rec["field"] = y.detach().clone()
        return y
    fu.F = types.SimpleNamespace(conv2d=conv2d)
    smoothing = fu.SoftErosion(kernel_size=KSIZE, threshold=THRESH, iterations=ITERS)

    def margin(lg):
        top = lg.topk(2, dim=1).values
        return (top[:, 0] - top[:, 1])[:, None]

    cases = [("face1368", demo_face("1368.jpg")), ("face7522", demo_face("7522.jpg")),
             ("synth128x96", synthetic_rgb(128, 96, 5)), ("tiny32", synthetic_rgb(32, 32, 11))]
    out, meta = {}, {"cases": [], "threshold": THRESH, "kernel_size": KSIZE, "iterations": ITERS, "margin_clip": MARGIN_CLIP,
                     "field_band": FIELD_BAND, "params": table,
                     "n_params": int(sum(v.numel() for v in probe.parameters()))}
    face_ids = [1, 2, 3, 4, 5, 6, 7, 10, 11, 12]
    with torch.no_grad():
        for name, rgb in cases:
            x = to_tensor(rgb)
            lab = train(x)
            mg = margin(logits["last"])
            scale = float(logits["last"].std())
            lab_e = evalm(x)
            mg_e = margin(logits["last"])
            enc = fu.encode_segmentation(lab)
            soft, hard = smoothing(enc[:, 0, None] + enc[:, 1, None])
            field = rec["field"]
            ids = sorted(set(lab.unique().tolist()))
            n_face = int(np.isin(lab.numpy(), face_ids).sum())
            assert len(ids) >= 5, (name, ids)
            assert 0 < n_face < lab.numel(), (name, n_face)
            assert lab.dtype == torch.int64 and tuple(lab.shape) == (1, 1) + rgb.shape[:2]
            flips = float((lab_e != lab).float().mean())
            out[f"{name}_rgb"] = rgb
            out[f"{name}_labels"] = lab[0, 0].numpy().astype(np.uint8)
            out[f"{name}_labels_eval"] = lab_e[0, 0].numpy().astype(np.uint8)
            # the tests only ask whether a margin is small: stored clipped at MARGIN_CLIP (keeps the file small)
            out[f"{name}_margin"] = np.minimum(mg[0, 0].numpy(), MARGIN_CLIP).astype(np.float32)
            out[f"{name}_margin_eval"] = np.minimum(mg_e[0, 0].numpy(), MARGIN_CLIP).astype(np.float32)
            # the thresholded field where it decides (within FIELD_BAND of the threshold; 0 elsewhere).  Everywhere else it
            # is implied by soft and hard: soft = field / (maximum below the threshold), checked here
            f0 = field[0, 0].numpy()
            out[f"{name}_field"] = np.where(np.abs(f0 - THRESH) <= FIELD_BAND, f0, 0).astype(np.float32)
            below = f0[f0 < THRESH]
            if below.size:
                mx = torch.from_numpy(below).max()
                implied = torch.where(torch.from_numpy(f0) >= THRESH, torch.ones(()), torch.from_numpy(f0) / mx)
                assert torch.equal(implied, soft[0, 0]), name
            out[f"{name}_soft"] = soft[0, 0].numpy().astype(np.float32)
            out[f"{name}_hard"] = hard[0, 0].numpy().astype(np.uint8)
            meta["cases"].append({"name": name, "H": rgb.shape[0], "W": rgb.shape[1], "classes": ids, "face_pixels": n_face,
                                  "hard_pixels": int(hard.sum()), "logit_std": scale, "eval_label_change": flips})
            print(f"{name}: {rgb.shape[:2]} classes {len(ids)} face {n_face} hard {int(hard.sum())} logit std {scale:.3f} "
                  f"eval changes {flips:.1%}")
    np.savez_compressed(os.path.join(HERE, "g17_face_parsing.npz"), **out)
    with open(os.path.join(HERE, "g17_face_parsing.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.join(HERE, "g17_face_parsing.npz"), os.path.getsize(os.path.join(HERE, "g17_face_parsing.npz")), "bytes")


if __name__ == "__main__":
    main()
