#!/usr/bin/env python3
"""Generate tests/golden/g18_baselines.npz + .json by RUNNING THE REFERENCE's comparison editors:
text-guided/inversion/p2p_baselines.py (ef_wo_p2p, ef_or_pnp_inv_w_p2p), masactrl_baselines.py
(ef_or_pnp_inv_w_masactrl) and pnp_baselines.py (negative_prompt_pnp, ef_or_pnp_inv_w_pnp), imported UNMODIFIED
through make_golden's stubs and driven with the seeded toys the other generators use.  Needs the reference tree, like
make_golden.py; the outputs are data only.

    python tests/golden/make_golden_baselines.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub, build_ref_controller, import_reference, npy  # noqa: E402

CFG = [1.0, 7.5]           # [cfg_src, cfg_tar] of the reference drivers' baseline modes


def gen_p2p(ref, d, meta):
    from helpers.tiny import PROMPT_PAIRS, ddim_tables, make_tiny_model
    import inversion.p2p_baselines as pb
    pb.tqdm = lambda x, *a, **k: x
    T = 10
    torch.manual_seed(1234)
    w0 = torch.randn(1, 4, 16, 16) * 0.8
    d["p2p_w0"] = npy(w0)
    inv = {}
    for pi in (0, 2):
        model = make_tiny_model(T)
        torch.manual_seed(4321 + pi)
        _, zs, wts, _ = ref.di.inversion_forward_process_ddpm(model, w0, etas=1.0, prog_bar=False, prompt=PROMPT_PAIRS[pi][0],
                                                              cfg_scale_src=1.0, num_inference_steps=T)
        inv["ddpm", pi] = (zs, wts)
        d[f"p2p_ddpm{pi}_zs"], d[f"p2p_ddpm{pi}_wts"] = npy(zs), npy(wts)
    model = make_tiny_model(T)
    model.scheduler = ddim_tables(T, steps_offset=0)
    _, zs, lats = ref.dd.ddim_inversion(model, w0, PROMPT_PAIRS[0][0], 1.0)
    inv["ddim", 0] = (zs, torch.stack([l[0] for l in lats]))
    d["p2p_ddim0_zs"], d["p2p_ddim0_wts"] = npy(zs), npy(inv["ddim", 0][1])

    def run(name, fn, kind, pi, skip, blend=True):
        model = make_tiny_model(T)
        if kind == "ddim":
            model.scheduler = ddim_tables(T, steps_offset=0)
        zs, wts = inv[kind, pi]
        after = T - skip
        pair = PROMPT_PAIRS[pi] if blend else PROMPT_PAIRS[pi][:2] + (None, PROMPT_PAIRS[pi][3])
        if fn == "ef_wo_p2p":
            ctrl = ref.pc.AttentionStore()
            prompts, cfg = [pair[1]], [CFG[1]]
        else:
            ctrl = build_ref_controller(ref, model, pair, after)
            prompts, cfg = [pair[0], pair[1]], CFG
        ref.pu.register_attention_control(model, ctrl)
        out = getattr(pb, fn)(model, xT=wts[after], etas=1.0, prompts=prompts, cfg_scales=cfg, prog_bar=False, zs=zs[:after],
                              controller=ctrl, is_ddim_inversion=(kind == "ddim"))
        case = {"name": name, "family": "p2p", "fn": fn, "inv": kind, "pair": pi, "skip": skip, "blend": blend,
                "cur_step": ctrl.cur_step, "single": isinstance(out, torch.Tensor)}
        if case["single"]:
            d[f"{name}_edit"] = npy(out)           # ef_wo_p2p returns one tensor
        else:
            d[f"{name}_edit"], d[f"{name}_recon"] = npy(out[0]), npy(out[1])
        meta.append(case)

    run("ef_skip3", "ef_wo_p2p", "ddpm", 0, 3)
    run("ef_p2p_skip0", "ef_or_pnp_inv_w_p2p", "ddpm", 0, 0)
    run("ef_p2p_skip3_noblend", "ef_or_pnp_inv_w_p2p", "ddpm", 2, 3, blend=False)
    run("pnp_inv_p2p", "ef_or_pnp_inv_w_p2p", "ddim", 0, 0)


def gen_masactrl(ref, d, meta):
    from helpers.tiny import PROMPT_PAIRS, ddim_tables, make_tiny_masa_model
    tv = _stub("torchvision")
    tv.utils = _stub("torchvision.utils", save_image=lambda *a, **k: None)
    import masactrl.masactrl_utils as mu
    pkg = _stub("masa_ctrl")
    pkg.masactrl_utils = mu
    sys.modules["masa_ctrl.masactrl_utils"] = mu
    import masactrl.masactrl as mm
    import inversion.masactrl_baselines as mb
    mb.tqdm = lambda x, *a, **k: x
    T = 10
    torch.manual_seed(1234)
    w0 = torch.randn(1, 4, 16, 16) * 0.8
    d["masa_w0"] = npy(w0)
    tar = PROMPT_PAIRS[0][1]
    for name, ddim, skip, step, layer in (("ef_masactrl", False, 0, 2, 3), ("pnp_inv_masactrl", True, 2, 1, 0)):
        model = make_tiny_masa_model(T)
        if ddim:
            model.scheduler = ddim_tables(T, steps_offset=0)
            _, zs, lats = ref.dd.ddim_inversion(model, w0, "", 1.0)
            wts = torch.stack([l[0] for l in lats])
        else:
            torch.manual_seed(4321)
            _, zs, wts, _ = ref.di.inversion_forward_process_ddpm(model, w0, etas=1.0, prog_bar=False, prompt="", cfg_scale_src=1.0,
                                                                  num_inference_steps=T)
        d[f"{name}_zs"], d[f"{name}_wts"] = npy(zs), npy(wts)
        model = make_tiny_masa_model(T)
        if ddim:
            model.scheduler = ddim_tables(T, steps_offset=0)
        editor = mm.MutualSelfAttentionControl(step, layer)
        mu.regiter_attention_editor_diffusers(model, editor)
        after = T - skip
        edit, recon = mb.ef_or_pnp_inv_w_masactrl(model, xT=wts[after], etas=1.0, prompts=["", tar], cfg_scales=CFG, prog_bar=False,
                                                  zs=zs[:after], is_ddim_inversion=ddim)
        d[f"{name}_edit"], d[f"{name}_recon"] = npy(edit), npy(recon)
        meta.append({"name": name, "family": "masactrl", "fn": "ef_or_pnp_inv_w_masactrl", "inv": "ddim" if ddim else "ddpm",
                     "skip": skip, "start_step": step, "start_layer": layer, "cur_step": editor.cur_step,
                     "num_att_layers": editor.num_att_layers, "single": False})


def gen_pnp(ref, d, meta):
    from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model
    import plug_n_play.pnp_utils as pu
    import inversion.pnp_baselines as pb
    pb.tqdm = lambda x, *a, **k: x
    T = 4
    torch.manual_seed(77)
    w0 = torch.randn(1, 4, 64, 64) * 0.8
    src, tar = PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]

    def fresh():
        model, _ = make_oracle_sd_model(TINY4_CONFIG, T)
        model.scheduler = ddim_tables(T, steps_offset=0)
        return model

    # one DDIM inversion for both cases: only w0 and the final latent are stored (the loops read zs for its length, and
    # with etas = 0 add none of it)
    _, zs, lats = ref.dd.ddim_inversion(fresh(), w0, src, 1.0)
    d["pnp_w0"], d["pnp_xT"] = npy(w0), npy(lats[T])
    for name, fn, f_t, attn_t in (("np_pnp", "negative_prompt_pnp", 0.5, 0.5), ("pnp_inv_pnp_eta0", "ef_or_pnp_inv_w_pnp", 0.5, 0.75)):
        model = fresh()
        n_f, n_a = int(T * f_t), int(T * attn_t)
        qk, conv = model.scheduler.timesteps[:n_a], model.scheduler.timesteps[:n_f]
        pu.register_attention_control_efficient(model, qk)
        pu.register_conv_control_efficient(model, conv)
        kw = dict(etas=0.0, prompts=[src, tar], cfg_scales=CFG, prog_bar=False, zs=zs[:T])
        if fn == "ef_or_pnp_inv_w_pnp":
            kw["is_ddim_inversion"] = True
        edit, recon = getattr(pb, fn)(model, xT=lats[T], **kw)
        d[f"{name}_edit"], d[f"{name}_recon"] = npy(edit), npy(recon)
        meta.append({"name": name, "family": "pnp", "fn": fn, "qk": [int(v) for v in qk], "conv": [int(v) for v in conv],
                     "single": False})


def main():
    torch.set_num_threads(4)
    ref = import_reference()
    d, meta = {}, []
    gen_p2p(ref, d, meta)
    gen_masactrl(ref, d, meta)
    gen_pnp(ref, d, meta)
    np.savez_compressed(os.path.join(HERE, "g18_baselines.npz"), **d)
    with open(os.path.join(HERE, "g18_baselines.json"), "w") as f:
        json.dump({"cfg": CFG, "cases": meta}, f, indent=0)
    for f in ("g18_baselines.npz", "g18_baselines.json"):
        print(f"{f:32s} {os.path.getsize(os.path.join(HERE, f)) / 1024:9.1f} KiB")


if __name__ == "__main__":
    main()
