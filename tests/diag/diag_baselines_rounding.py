"""Diagnostic (not collected by pytest; CPU only): which term makes the comparison editors more sensitive to the storage
format than the h-Edit loops.  The fp32 twins (tests/helpers/baseline_ref.py) and the oracle's h-Edit loop run twice on
the SAME network, inversion and injection schedule -- plain, and with every UNet output rounded to a 16-bit format (one
rounding per eps evaluation: a LOWER bound of what a 16-bit activation path does) -- and the relative L2 of the final
latents between the two runs is printed, with the guidance weight the loop applies to the whole eps.

    python tests/diag/diag_baselines_rounding.py [bf16|f16]

The direct samplers multiply the whole noise prediction of the target row by cfg_tar (x_next takes
e_u + 7.5 (e_c - e_u): independent rounding errors of e_u and e_c enter with weights 6.5 and 7.5), negative-prompt
inversion does so for the source row as well; h-Edit steps both rows with cfg_src = 1 and adds the guided difference
only through the small edit coefficient."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "h-edit_amd")):
    sys.path.insert(0, p)
from helpers import baseline_ref as BR  # noqa: E402
from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model  # noqa: E402
from oracle import loops as OL  # noqa: E402
from oracle import pnp as OPNP  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def model(T, dtype):
    m, _ = make_oracle_sd_model(TINY4_CONFIG, T)
    m.scheduler = ddim_tables(T, steps_offset=0)
    OPNP.register_pnp(m, [int(t) for t in m.scheduler.timesteps[:2]], [int(t) for t in m.scheduler.timesteps[:2]])
    if dtype is not None:
        plain = m.unet.forward

        def rounded(*a, **k):
            out = plain(*a, **k)
            out["sample"] = out["sample"].to(dtype).float()
            return out
        m.unet.forward = rounded
    return m


def main():
    dtype = torch.float16 if "f16" in sys.argv[1:] else torch.bfloat16
    torch.set_num_threads(8)
    T = 4
    src, tar = PROMPT_PAIRS[0][:2]
    torch.manual_seed(77)
    w0 = torch.randn(1, 4, 64, 64) * 0.8
    base, _ = make_oracle_sd_model(TINY4_CONFIG, T)
    base.scheduler = ddim_tables(T, steps_offset=0)
    _, zs, lats = OL.ddim_inversion(base, w0, src, 1.0)
    xT = lats[T]
    runs = {
        "negative_prompt_pnp   (cfg 7.5 on both rows)": lambda m: BR.negative_prompt_pnp(m, xT, etas=0.0, prompts=[src, tar], cfg_scales=[1.0, 7.5], zs=zs),
        "ef_or_pnp_inv_w_pnp   (cfg 1 / 7.5)": lambda m: BR.ef_or_pnp_inv_w_pnp(m, xT, etas=0.0, prompts=[src, tar], cfg_scales=[1.0, 7.5], zs=zs,
                                                                                 is_ddim_inversion=True),
        "h_edit_pnp_implicit   (cfg 1 step + coeff * guided difference)": lambda m: OL.h_edit_pnp_implicit(
            m, xT, eta=1.0, prompts=[src, tar], cfg_scales=[1.0, 5.0, 7.5], zs=zs, optimization_steps=1, after_skip_steps=T,
            is_ddim_inversion=True),
    }
    for name, fn in runs.items():
        e0, r0 = fn(model(T, None))
        e1, r1 = fn(model(T, dtype))
        print(f"{str(dtype):16s} {name:66s} edit {rel(e1, e0):.3e}  recon {rel(r1, r0):.3e}", flush=True)


if __name__ == "__main__":
    main()
