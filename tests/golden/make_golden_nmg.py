#!/usr/bin/env python3
"""Generate tests/golden/g22_nmg.npz + .json by RUNNING THE REFERENCE's Noise Map Guidance loops:
text-guided/inversion/p2p_baselines.py (nmg_p2p) and pnp_baselines.py (nmg_pnp), imported UNMODIFIED through
make_golden's stubs and driven with the seeded toys of make_golden_baselines.py.  Needs the reference tree, like
make_golden.py; the outputs are data only.

    python tests/golden/make_golden_nmg.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_ref_controller, import_reference, npy  # noqa: E402

CFG = [1.0, 7.5]           # [cfg_src, cfg_tar] of the reference drivers' NMG modes
NMG = dict(guidance_noise_map=10.0, grad_scale=5e+3)      # main_p2p.py:240


def gen_p2p(ref, d, meta):
    from helpers.tiny import PROMPT_PAIRS, ddim_tables, make_tiny_model
    import inversion.p2p_baselines as pb
    pb.tqdm = lambda x, *a, **k: x
    T = 10
    torch.manual_seed(1234)
    w0 = torch.randn(1, 4, 16, 16) * 0.8
    d["p2p_w0"] = npy(w0)

    def fresh():
        model = make_tiny_model(T)
        model.scheduler = ddim_tables(T, steps_offset=0)
        return model

    inv = {}
    for pi in (0, 2):
        _, zs, lats = ref.dd.ddim_inversion(fresh(), w0, PROMPT_PAIRS[pi][0], 1.0)
        inv[pi] = (zs, torch.stack(list(lats)))               # (T, 1, C, H, W), (T + 1, 1, C, H, W)
        d[f"p2p_inv{pi}_zs"], d[f"p2p_inv{pi}_wts"] = npy(inv[pi][0]), npy(inv[pi][1])

    def run(name, pi, skip, p2p, blend=True):
        model = fresh()
        zs, wts = inv[pi]
        after = T - skip
        pair = PROMPT_PAIRS[pi] if blend else PROMPT_PAIRS[pi][:2] + (None, PROMPT_PAIRS[pi][3])
        # `nmg`: what main_p2p.py:238 dispatches -- the plain store (the name does not end in p2p, :187-205)
        ctrl = build_ref_controller(ref, model, pair, after) if p2p else ref.pc.AttentionStore()
        ref.pu.register_attention_control(model, ctrl)
        edit, recon = pb.nmg_p2p(model, xT=wts[after], xT_ori=wts[:after + 1], etas=0.0, prompts=[pair[0], pair[1]], cfg_scales=CFG,
                                 prog_bar=False, zs=zs[:after], controller=ctrl, **NMG)
        d[f"{name}_edit"], d[f"{name}_recon"] = npy(edit), npy(recon)
        meta.append({"name": name, "family": "p2p", "fn": "nmg_p2p", "pair": pi, "skip": skip, "p2p": p2p, "blend": blend,
                     "cur_step": ctrl.cur_step})

    run("nmg_store_skip0", 0, 0, False)
    run("nmg_p2p_skip0", 0, 0, True)
    run("nmg_p2p_skip3_noblend", 2, 3, True, blend=False)
    run("nmg_p2p_skip3", 0, 3, True)


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

    _, zs, lats = ref.dd.ddim_inversion(fresh(), w0, src, 1.0)
    wts = torch.stack(list(lats))
    d["pnp_w0"], d["pnp_wts"] = npy(w0), npy(wts)
    model = fresh()
    n_f, n_a = int(T * 0.5), int(T * 0.75)
    qk, conv = model.scheduler.timesteps[:n_a], model.scheduler.timesteps[:n_f]
    pu.register_attention_control_efficient(model, qk)
    pu.register_conv_control_efficient(model, conv)
    edit, recon = pb.nmg_pnp(model, xT=wts[T], xT_ori=wts[:T + 1], etas=0.0, prompts=[src, tar], cfg_scales=CFG, prog_bar=False,
                             zs=zs[:T], **NMG)
    d["nmg_pnp_edit"], d["nmg_pnp_recon"] = npy(edit), npy(recon)
    meta.append({"name": "nmg_pnp", "family": "pnp", "fn": "nmg_pnp", "qk": [int(v) for v in qk], "conv": [int(v) for v in conv]})


def main():
    torch.set_num_threads(4)
    ref = import_reference()
    d, meta = {}, []
    gen_p2p(ref, d, meta)
    gen_pnp(ref, d, meta)
    np.savez_compressed(os.path.join(HERE, "g22_nmg.npz"), **d)
    with open(os.path.join(HERE, "g22_nmg.json"), "w") as f:
        json.dump({"cfg": CFG, "nmg": NMG, "T": 10, "T_pnp": 4, "cases": meta}, f, indent=0)
    for f in ("g22_nmg.npz", "g22_nmg.json"):
        print(f"{f:32s} {os.path.getsize(os.path.join(HERE, f)) / 1024:9.1f} KiB")


if __name__ == "__main__":
    main()
