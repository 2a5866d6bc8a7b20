#!/usr/bin/env python3
"""Generate tests/golden/g24_nulltext.npz + .json by RUNNING THE REFERENCE's null-text inversion with Plug-and-Play:
text-guided/inversion/pnp_baselines.py (nulltext_pnp :134-236), imported UNMODIFIED through make_golden's stubs and driven
with the four-level toy of make_golden_nmg.py (32 x 32 latents, 4 steps, 4 threads, the reference's own injection hooks registered).  Needs
the reference tree, like make_golden.py; the outputs are data only.

Besides (edit, recon) every case records what the inner optimisation did: the number of Adam updates taken per step and
every inner loss.  The function's text is not touched for that: the name `F` of the reference module's namespace is bound to an
object whose `mse_loss` records and forwards, and `register_time` (called once per step) is wrapped to open a new row.

    python tests/golden/make_golden_nt.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy  # noqa: E402

CFG = [1.0, 7.5]           # [cfg_src, cfg_tar] of the reference driver's nt_pnp mode
T = 4
# (name, optimization_steps, epsilon).  `stops`: epsilon sits between the first inner losses of the four steps (printed by this
# script for the `full` case), so the reference's stop `loss < epsilon + i * 2e-5` ends some steps after one update and lets the
# others run out
CASES = [("full", 2, 1e-5), ("stops", 2, None)]


class RecordingF:
    def __init__(self, rows):
        self.rows = rows

    def mse_loss(self, a, b, *args, **kw):
        loss = torch.nn.functional.mse_loss(a, b, *args, **kw)
        self.rows[-1].append(float(loss.detach()))
        return loss

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


def main():
    torch.set_num_threads(4)
    ref = import_reference()
    from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model
    import plug_n_play.pnp_utils as pu
    import inversion.pnp_baselines as pb
    pb.tqdm = lambda x, *a, **k: x
    tell_time = pb.register_time
    torch.manual_seed(77)
    w0 = torch.randn(1, 4, 32, 32) * 0.8      # the torch toy takes any size divisible by 8: a quarter of the work of 64 x 64
    src, tar = PROMPT_PAIRS[0][0], PROMPT_PAIRS[0][1]

    def fresh():
        model, _ = make_oracle_sd_model(dict(TINY4_CONFIG, sample_size=32), T)
        model.scheduler = ddim_tables(T, steps_offset=0)
        return model

    _, zs, lats = ref.dd.ddim_inversion(fresh(), w0, src, 1.0)
    wts = torch.stack(list(lats))
    d, meta = {"w0": npy(w0), "wts": npy(wts)}, []
    eps_stops = None
    for name, steps, epsilon in CASES:
        if epsilon is None:
            epsilon = eps_stops
        model = fresh()
        n_f, n_a = int(T * 0.5), int(T * 0.75)
        qk, conv = model.scheduler.timesteps[:n_a], model.scheduler.timesteps[:n_f]
        pu.register_attention_control_efficient(model, qk)
        pu.register_conv_control_efficient(model, conv)
        rows = []

        def rt(m, t):
            rows.append([])
            return tell_time(m, t)

        pb.F, pb.register_time = RecordingF(rows), rt
        try:
            edit, recon = pb.nulltext_pnp(model, xT=wts[T], xT_ori=wts[:T + 1], etas=0.0, prompts=[src, tar], cfg_scales=CFG,
                                          prog_bar=False, zs=zs[:T], optimization_steps=steps, epsilon=epsilon)
        finally:
            pb.F, pb.register_time = torch.nn.functional, tell_time
        d[f"{name}_edit"], d[f"{name}_recon"] = npy(edit), npy(recon)
        meta.append({"name": name, "optimization_steps": steps, "epsilon": epsilon, "updates": [len(r) for r in rows], "losses": rows,
                     "qk": [int(v) for v in qk], "conv": [int(v) for v in conv],
                     "decreases": bool(any(len(r) > 1 and r[-1] < r[0] for r in rows))})
        print(name, "epsilon", epsilon, "updates", [len(r) for r in rows])
        for r in rows:
            print("   ", " ".join(f"{v:.6e}" for v in r))
        if eps_stops is None:
            # between the two middle values of (first loss of step i) - i * 2e-5: two steps stop at once, two do not
            firsts = sorted(r[0] - i * 2e-5 for i, r in enumerate(rows))
            eps_stops = float(np.float32(0.5 * (firsts[1] + firsts[2])))
    np.savez_compressed(os.path.join(HERE, "g24_nulltext.npz"), **d)
    with open(os.path.join(HERE, "g24_nulltext.json"), "w") as f:
        json.dump({"cfg": CFG, "T": T, "cases": meta}, f, indent=0)
    for f in ("g24_nulltext.npz", "g24_nulltext.json"):
        print(f"{f:32s} {os.path.getsize(os.path.join(HERE, f)) / 1024:9.1f} KiB")


if __name__ == "__main__":
    main()
