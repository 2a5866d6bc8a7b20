"""Host-side behaviour of the comparison editors that needs no GPU: what the driver refuses and why, the eta each mode
asks for, and the reference's assertions in the reference-signature functions (they fire before any device work)."""
import importlib.util
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver():
    spec = importlib.util.spec_from_file_location("hedit_main_baselines", os.path.join(ROOT, "h-edit_amd", "main_baselines.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("mode,why", [("nmg_p2p", "gradient"), ("nmg_pnp", "gradient"), ("nt_pnp", "gradient"), ("ef_pnp", "etas == 0"),
                                      ("pnp_inv_w_pnp", "etas == 0"), ("h_edit_R_p2p", "own drivers")])
def test_driver_says_why_it_refuses(mode, why):
    with pytest.raises(NotImplementedError) as ei:
        _driver().main(["--mode", mode])
    assert mode in str(ei.value) and why in str(ei.value)


def test_driver_modes_and_their_eta():
    d = _driver()
    assert set(d.MODES) == {"ef", "ef_p2p", "pnp_inv_p2p", "ef_masactrl", "pnp_inv_masactrl", "np_pnp"}
    for mode, (_, eta) in d.MODES.items():
        assert eta == (0.0 if mode.startswith(("pnp_inv", "np_")) else 1.0)
        with pytest.raises(AssertionError):
            d.main(["--mode", mode, "--eta", str(1.0 - eta)])


def test_reference_assertions_are_kept():
    from hedit.inversion import masactrl_baselines as MB
    from hedit.inversion import p2p_baselines as PB
    from hedit.inversion import pnp_baselines as NB
    model = types.SimpleNamespace(scheduler=types.SimpleNamespace(num_inference_steps=4))
    with pytest.raises(AssertionError):
        PB.ef_or_pnp_inv_w_p2p(model, None, prompts=["only one"], cfg_scales=[1.0, 7.5])
    with pytest.raises(AssertionError):
        MB.ef_or_pnp_inv_w_masactrl(model, None, prompts=["only one"], cfg_scales=[1.0, 7.5])
    for fn in (NB.negative_prompt_pnp, NB.ef_or_pnp_inv_w_pnp):
        with pytest.raises(AssertionError):                       # etas must be 0 (pnp_baselines.py:264, :338)
            fn(model, None, etas=1.0, prompts=["a", "b"], cfg_scales=[1.0, 7.5])
        with pytest.raises(AssertionError):
            fn(model, None, etas=0, prompts=["a"], cfg_scales=[1.0, 7.5])
    with pytest.raises(AssertionError):                           # one eta per inference step
        PB._etas(model, [1.0, 1.0])
    assert PB._etas(model, None) == 0.0 and PB._etas(model, 1) == 1.0 and PB._etas(model, [1.0, 0.5, 1.0, 1.0]) == [1.0, 0.5, 1.0, 1.0]
