#!/usr/bin/env python3
"""Generate tests/golden/g26_ef_style.npz + .json by RUNNING THE REFERENCE's Edit Friendly loop of the combined text + style
task: text-guided-n-style/inversion/ef.py (ef_p2p), imported UNMODIFIED through make_golden's stubs and driven with the
seeded toys of g9 (tests/helpers/tiny.py: make_tiny_model + TinyVae + TinyStyleEncoder, T = 10, 16 x 16).  In its own
interpreter, like make_golden.py --style-child: the n-style sub-project reuses the package names ``inversion`` / ``p2p`` of
text-guided.  Needs the reference tree; the outputs are data only.  ``autocast("cuda")`` inside the loop is disabled with a
warning on a machine without a GPU.

Every case is checked to stay well conditioned: the reference's edit must stay below 3 x rms(w0) = 2.39.  On these toys it is
the text edit at cfg_tar = 7.5 that leaves the range, not the style step, so the skip decides and the weight hardly does --
measured: pair 2 with blend, skip 3: 3.6 / 3.0 at weight 0.5 / 1.5, skip 5: 1.6 / 1.8; pair 0 without blend, skip 0: 5.5 /
6.6 / 7.1 at weight 0.1 / 0.4 / 1.5 (no other pair stays below 9 there), skip 4: 2.8, skip 6: 1.0; pair 0 under
is_ddim_inversion, skip 3: 3.1 / 3.4, skip 6: 1.4 / 1.6.  Hence no case at skip 0: the case without a blend word has skip 6.

    python tests/golden/make_golden_ef_style.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_STYLE, _stub, build_ref_controller, npy  # noqa: E402

CFG = [1.0, 7.5]           # [cfg_src, cfg_tar]: two entries (main_edit.py:218-223)
T = 10
# (name, pair, skip, weight_edit_clip, blend word, is_ddim_inversion)
CASES = [("ef_blend_skip5", 2, 5, 1.5, True, False),
         ("ef_noblend_skip6", 0, 6, 0.5, False, False),
         ("ef_blend_skip6_ddim", 0, 6, 1.5, True, True)]


def import_reference():
    if not os.path.isdir(REF_STYLE):
        raise SystemExit("reference tree not present; golden vectors can only be (re)generated in the build container")
    _stub("diffusers")
    _stub("diffusers.utils")
    _stub("diffusers.utils.torch_utils", randn_tensor=None)
    _stub("diffusers.models")
    _stub("diffusers.models.attention_processor", Attention=object)
    _stub("cv2")
    nltk = _stub("nltk", download=lambda *a, **k: None)
    nltk.tokenize = _stub("nltk.tokenize", word_tokenize=lambda s: s.split())
    sys.path.insert(0, REF_STYLE)
    warnings.filterwarnings("ignore")
    import inversion.ddpm_inversion as di
    import inversion.ef as ef
    import p2p.ptp_classes as pc
    import p2p.ptp_controller_utils as pcu
    import p2p.ptp_utils as pu
    ef.tqdm = lambda x, *a, **k: x
    di.tqdm = lambda x, *a, **k: x
    return types.SimpleNamespace(ef=ef, di=di, pc=pc, pcu=pcu, pu=pu)


def main():
    torch.set_num_threads(4)
    ref = import_reference()
    from helpers.tiny import PROMPT_PAIRS, TinyStyleEncoder, TinyVae, make_tiny_model
    torch.manual_seed(1234)                 # the g3 / g9 start sample
    w0 = torch.randn(1, 4, 16, 16) * 0.8
    d, meta = {"w0": npy(w0)}, []
    rms0 = float(w0.pow(2).mean().sqrt())

    def fresh():
        model = make_tiny_model(T)
        model.vae = TinyVae()
        return model

    for name, pi, skip, weight, blend, ddim in CASES:
        torch.manual_seed(4321 + pi)
        _, zs, wts, _ = ref.di.inversion_forward_process_ddpm(fresh(), w0, etas=1.0, prog_bar=False, prompt=PROMPT_PAIRS[pi][0],
                                                              cfg_scale_src=1.0, num_inference_steps=T)
        model = fresh()
        after = T - skip
        pair = PROMPT_PAIRS[pi] if blend else PROMPT_PAIRS[pi][:2] + (None, PROMPT_PAIRS[pi][3])
        ctrl = build_ref_controller(ref, model, pair, after)
        ref.pu.register_attention_control(model, ctrl)
        edit, recon = ref.ef.ef_p2p(model, TinyStyleEncoder(), xT=wts[after], etas=1.0, prompts=[pair[0], pair[1]], cfg_scales=CFG,
                                    prog_bar=False, zs=zs[:after], controller=ctrl, weight_edit_clip=weight,
                                    is_ddim_inversion=ddim)
        rms = float(edit.pow(2).mean().sqrt())
        assert torch.isfinite(edit).all() and torch.isfinite(recon).all(), name
        assert rms < 3 * rms0, f"{name}: edit rms {rms:.3f} against {rms0:.3f} for w0 -- lower the weight or add skip"
        print(f"{name:24s} edit rms {rms:.3f}  recon rms {float(recon.pow(2).mean().sqrt()):.3f}  (w0 {rms0:.3f})")
        d[f"{name}_zs"], d[f"{name}_wts"] = npy(zs), npy(wts)
        d[f"{name}_edit"], d[f"{name}_recon"] = npy(edit), npy(recon)
        meta.append({"name": name, "pair": pi, "skip": skip, "weight": weight, "blend": blend, "ddim": ddim,
                     "cur_step": ctrl.cur_step, "edit_rms": rms})
    np.savez_compressed(os.path.join(HERE, "g26_ef_style.npz"), **d)
    with open(os.path.join(HERE, "g26_ef_style.json"), "w") as f:
        json.dump({"cfg": CFG, "T": T, "w0_rms": rms0, "cases": meta}, f, indent=0)
    for f in ("g26_ef_style.npz", "g26_ef_style.json"):
        print(f"{f:32s} {os.path.getsize(os.path.join(HERE, f)) / 1024:9.1f} KiB")


if __name__ == "__main__":
    main()
