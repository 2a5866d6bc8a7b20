"""No GPU: null-text inversion with Plug-and-Play (hedit.inversion.pnp_baselines.nulltext_pnp) on the four-level torch toy of
tests/helpers/tiny.py against tests/golden/g24_nulltext.npz -- the reference's own function, run unmodified by
tests/golden/make_golden_nt.py on the same toy (32 x 32 latents, 4 steps, 2 inner updates at the most, the oracle's injection hooks, which are
pinned on the reference's).  Both sides do the same torch-CPU arithmetic through the autograd of the same network, so the limits
are those of tests/test_host_nmg.py: atol 5e-4, rtol 1e-4, at the generator's 4 threads.  The inner loop is compared too: the
number of Adam updates per step (one case's epsilon sits between the steps' first losses, so the reference's stop ends two steps
after one update and lets two run out) and every inner loss.

Also here: the lock-step form (one embedding, one optimiser, one loss per image; an image that met the stop is frozen), the
reference's assertions, and what main_nt.py runs and refuses."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.tiny import PROMPT_PAIRS, TINY4_CONFIG, ddim_tables, make_oracle_sd_model, make_tiny_model  # noqa: E402
import hedit.inversion.pnp_baselines as PB  # noqa: E402
from oracle import pnp as ON  # noqa: E402
from test_host_nmg import ElementwiseUNet  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def generator_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)          # make_golden_nt.py's
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "g24_nulltext.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "g24_nulltext.npz")), meta


class RecordingF:
    """what make_golden_nt.py binds to the reference module's `F`: every mse_loss goes into the row of the current step"""

    def __init__(self, rows):
        self.rows = rows

    def mse_loss(self, a, b, *args, **kw):
        loss = torch.nn.functional.mse_loss(a, b, *args, **kw)
        self.rows[-1].append(float(loss.detach()))
        return loss


def recorded(monkeypatch, tell_time):
    """-> (rows, register_time): rows[i] = the inner losses of step i, in call order"""
    rows = []
    monkeypatch.setattr(PB, "F", RecordingF(rows))

    def rt(model, t):
        rows.append([])
        return tell_time(model, t)

    return rows, rt


@pytest.mark.parametrize("ci", range(2))
def test_nulltext_pnp_matches_the_reference(gold, monkeypatch, ci):
    g, meta = gold
    case = meta["cases"][ci]
    T = meta["T"]
    model, _ = make_oracle_sd_model(dict(TINY4_CONFIG, sample_size=32), T)
    model.scheduler = ddim_tables(T, steps_offset=0)
    ON.register_pnp(model, case["qk"], case["conv"])
    wts = torch.from_numpy(g["wts"])
    rows, rt = recorded(monkeypatch, ON.register_time)
    edit, recon = PB.nulltext_pnp(model, xT=wts[T], xT_ori=wts[:T + 1], etas=0.0, prompts=list(PROMPT_PAIRS[0][:2]), cfg_scales=meta["cfg"],
                                  zs=torch.zeros(T, 1), optimization_steps=case["optimization_steps"], epsilon=case["epsilon"],
                                  register_time=rt)
    assert edit.shape == recon.shape == (1, 4, 32, 32)
    assert [len(r) for r in rows] == case["updates"]
    if case["name"] == "stops":
        assert 1 in case["updates"] and case["optimization_steps"] in case["updates"]      # the stop triggers in some steps only
    for got, want in zip(rows, case["losses"]):
        assert np.allclose(got, want, atol=5e-4, rtol=1e-4), (got, want)
    for name, got in (("edit", edit), ("recon", recon)):
        want = g[f"{case['name']}_{name}"]
        assert np.allclose(got.detach().numpy(), want, atol=5e-4, rtol=1e-4), float(np.abs(got.detach().numpy() - want).max())


def test_lock_step_freezes_an_image_that_met_the_stop(gold, monkeypatch):
    """Entry j of a per_image batch is its single run, bit for bit, over four steps, on test_host_nmg's elementwise eps-model
    (its eps depends on the context mean, so it is differentiable in the context; a matrix product on the CPU would not promise
    batch-invariant bits).  epsilon lies between the two images' first losses of step 0, so one image stops after a single update
    there while the other runs on: the update counts of the batch are the two single runs' interleaved."""
    g, _ = gold
    T, after = 10, 4
    nmg = np.load(os.path.join(GOLD, "g22_nmg.npz"))
    wts = torch.cat([torch.from_numpy(nmg["p2p_inv0_wts"]), torch.from_numpy(nmg["p2p_inv2_wts"])], dim=1)       # (T + 1, 2, C, H, W)
    pairs = [list(PROMPT_PAIRS[0][:2]), list(PROMPT_PAIRS[2][:2])]

    def run(sel, epsilon, per_image=True):
        model = make_tiny_model(T)
        model.scheduler = ddim_tables(T, steps_offset=0)
        model.unet = ElementwiseUNet()
        model.text_encoder = lambda ids: (torch.sin(ids.float()).unsqueeze(-1).expand(-1, -1, 8),)      # a lookup: no matrix product
        model.tokenizer([w for pr in pairs for w in pr], padding="max_length", max_length=model.tokenizer.model_max_length,
                        truncation=True, return_tensors="pt")
        rows, rt = recorded(monkeypatch, lambda m, t: None)
        p = [pairs[j] for j in sel]
        out = PB.nulltext_pnp(model, xT=wts[after][sel], xT_ori=wts[:after + 1][:, sel], etas=0.0, prompts=p if len(p) > 1 else p[0],
                              cfg_scales=[1.0, 7.5], zs=torch.zeros(after, 1), optimization_steps=3, epsilon=epsilon,
                              per_image=per_image, register_time=rt)
        return out, rows

    first = [run([j], 1e-5)[1][0][0] for j in (0, 1)]
    assert first[0] != first[1]
    epsilon = 0.5 * (first[0] + first[1])
    both, rows_both = run([0, 1], epsilon)
    counts = []
    for j in (0, 1):
        one, rows = run([j], epsilon)
        plain, _ = run([j], epsilon, per_image=False)
        counts.append([len(r) for r in rows])
        for b, o, q in zip(both, one, plain):
            assert torch.isfinite(o).all() and torch.equal(b[j:j + 1], o), j
            assert torch.equal(o, q)                          # one image: the per-image loss IS the reference's
    assert counts[0][0] != counts[1][0] and 1 in (counts[0][0], counts[1][0])          # one stopped at once, the other did not
    assert [len(r) for r in rows_both] == [a + b for a, b in zip(*counts)]
    with pytest.raises(ValueError, match="per_image"):
        run([0, 1], epsilon, per_image=False)


def test_reference_assertions_are_kept():
    model = types.SimpleNamespace(scheduler=types.SimpleNamespace(num_inference_steps=4))
    with pytest.raises(AssertionError):                   # etas must be 0 (pnp_baselines.py:162)
        PB.nulltext_pnp(model, None, None, etas=1.0, prompts=["a", "b"], cfg_scales=[1.0, 7.5])
    with pytest.raises(AssertionError):                   # two prompts
        PB.nulltext_pnp(model, None, None, etas=0, prompts=["a"], cfg_scales=[1.0, 7.5])
    import inspect
    sig = inspect.signature(PB.nulltext_pnp)
    assert list(sig.parameters) == ["model", "xT", "xT_ori", "etas", "prompts", "cfg_scales", "prog_bar", "zs", "optimization_steps",
                                    "epsilon", "per_image", "register_time"]
    assert sig.parameters["optimization_steps"].default == 10 and sig.parameters["epsilon"].default == 1e-5
    assert "not provided" not in PB.__doc__ and "nulltext_pnp" in PB.__doc__


def _driver(name):
    spec = importlib.util.spec_from_file_location("hedit_" + name, os.path.join(ROOT, "h-edit_amd", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_driver_modes_and_refusals():
    d = _driver("main_nt")
    assert d.MODES == {"nt_pnp": "pnp"} and d.NT == {"optimization_steps": 10}
    for mode, where in (("nmg_pnp", "main_nmg.py"), ("nmg", "main_nmg.py"), ("np_pnp", "main_baselines.py"), ("h_edit_R_pnp", "h-Edit drivers")):
        with pytest.raises(NotImplementedError) as ei:
            d.main(["--mode", mode])
        assert mode in str(ei.value) and where in str(ei.value)
    with pytest.raises(AssertionError):                       # null-text inversion is deterministic: the DDIM inversion, eta = 0
        d.main(["--mode", "nt_pnp", "--eta", "1.0"])


@pytest.mark.parametrize("name,words", [("main_nmg", ("nt_pnp", "context", "gradient", "main_nt.py")),
                                        ("main_baselines", ("nt_pnp", "gradient", "main_nt.py"))])
def test_the_older_drivers_say_where_nt_pnp_runs(name, words):
    with pytest.raises(NotImplementedError) as ei:
        _driver(name).main(["--mode", "nt_pnp"])
    for w in words:
        assert w in str(ei.value), w


def test_new_exports_are_declared():
    """the C header and the library's ctypes table both carry the new entry points (tests/test_host_p2p.py checks that the
    two agree as a whole and that the built library exports every name)"""
    from hedit import _lib
    with open(os.path.join(ROOT, "include", "hedit.h")) as f:
        header = f.read()
    for n in ("hedit_k_cross_attn_bwd_kv_ws_bytes", "hedit_k_cross_attn_bwd_kv", "hedit_unet_create_grad_ctx", "hedit_unet_backward_ctx"):
        assert n + "(" in header and n in _lib.EXPORTS, n
