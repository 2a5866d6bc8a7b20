"""-m gpu: native SqueezeNet-LPIPS (hedit_sqlpips_* of csrc/sqlpips.hip behind hedit.lpips_score.NativeSqueezeLpips) and
the evaluator's lpips columns, on seeded stand-in weights, against the fp64 torch restatement tests/helpers/sqlpips_ref.py
run on the CPU.  PARITY UNPINNED: torchvision, lpips and torchmetrics are not installed here and the reference tree holds
no vector for this metric; what is checked is the native executor against the restatement (whose tap sizes
tests/test_host_sqlpips.py pins to the published network's).

Limit: |native - ref| <= 1e-5 |ref| + 1e-9, the project's LPIPS limit (tests/test_gpu_lpips.py).  torch's own fp32
restatement sits within 3.2e-7 (relative) of fp64 on these inputs, so the limit leaves >= 30 x over the reference arithmetic.
Batch, argument-order, repeat and storage-format comparisons are bit for bit.

MEASURED (MI355X, bfloat16 build; every parity test prints its figures with -s before it asserts), |native - ref| / |ref|:
  34 x 46 whole 8.4e-8, masked 7.6e-8;  36 x 52 3.1e-8 / 3.5e-8;  64 x 64 1.8e-7 / 1.6e-7;  128 x 96 6.0e-8 / 6.0e-8
  512 x 512 1.1e-8;  squeeze biases of +1: 3.1e-8 ... 1.6e-7
Wall time of the file: 4.5 s inside pytest, of which the child process in the other storage build 2.0 s.
"""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import gpu as G  # noqa: E402
from helpers import sqlpips_child as SC  # noqa: E402
from helpers import sqlpips_ref as SR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.lpips_score import MAX_BATCH, NativeSqueezeLpips, SqueezeLpipsNet, preprocess_pair  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((34, 46), (36, 52), (64, 64), (128, 96))


def _within(native, ref, what):
    native, ref = float(native), float(ref)
    err = abs(native - ref)
    print(f"[sqlpips parity] {what}: native {native:.9e} ref {ref:.9e} |diff| {err:.3e} = {err / max(abs(ref), 1e-300):.3e} relative")
    assert err <= 1e-5 * abs(ref) + 1e-9, (what, native, ref)


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return NativeSqueezeLpips(device=G.dev(), seed=SC.SEED)


def _whole_and_masked(H, W, seed):
    a8, b8 = SR.uint8_pair(H, W, seed)
    m = SR.upper_half_mask(H, W)
    p = [preprocess_pair(a8, b8), preprocess_pair(a8, b8, m, m)]
    return torch.stack([x[0] for x in p]), torch.stack([x[1] for x in p])


@pytest.mark.parametrize("H,W", SIZES)
def test_parity_with_the_fp64_restatement(model, H, W):
    """34 x 46 and 36 x 52 meet a partial pooling window at every pool, 64 x 64 ends in 3 x 3 maps, 128 x 96 has several
    tiles per map; each whole and with the upper half masked"""
    a, b = _whole_and_masked(H, W, 100 + H)
    ref = SR.distance(model.net.params, a, b)
    got = model.distance(a.to(G.dev()), b.to(G.dev())).cpu()
    for i, tag in enumerate(("whole", "upper half masked")):
        _within(got[i], ref[i], f"{H}x{W} {tag}")
    assert float(ref[0]) > 0 and float(ref[1]) > 0 and float(ref[0]) != float(ref[1])


def test_parity_at_the_pie_bench_shape(model):
    """one 512 x 512 pair: 255 x 255 / 127 x 127 / 63 x 63 / 31 x 31 maps, many tiles, no partial pooling window"""
    a8, b8 = SR.uint8_pair(512, 512, 9)
    a, b = preprocess_pair(a8, b8)
    ref = SR.distance(model.net.params, a[None], b[None])
    got = model.distance(a[None].to(G.dev()), b[None].to(G.dev())).cpu()
    _within(got[0], ref[0], "512x512")


def test_the_padding_of_expand3x3_is_zero_not_relu_of_the_bias():
    """squeeze biases of +1: a squeeze map padded with relu(bias) = 1 instead of 0 moves every border pixel of every Fire
    module, far beyond the limit (small maps are mostly border)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    net = SqueezeLpipsNet().init_random(4)
    sd = {k: (torch.ones_like(v) if k.endswith("squeeze.bias") else v) for k, v in net.state_dict().items()}
    m = NativeSqueezeLpips(sd, device=G.dev())
    for H, W in ((34, 46), (64, 64)):
        a, b = _whole_and_masked(H, W, 40 + H)
        ref = SR.distance(m.net.params, a, b)
        got = m.distance(a.to(G.dev()), b.to(G.dev())).cpu()
        for i in range(2):
            _within(got[i], ref[i], f"squeeze bias +1, {H}x{W} [{i}]")


@pytest.mark.parametrize("N", [3, 5])
def test_a_batch_gives_the_bits_of_single_calls(model, N):
    for H, W in ((36, 52), (128, 96)):
        a, b = SC.pairs(H, W, N, seed0=500 + N)
        a, b = a.to(G.dev()), b.to(G.dev())
        n0 = model.calls
        batch = model.distance(a, b)
        assert model.calls == n0 + 1
        single = torch.cat([model.distance(a[i:i + 1], b[i:i + 1]) for i in range(N)])
        G.sync()
        assert torch.equal(batch, single), (H, W, batch, single)
        assert torch.equal(model.distance(b, a), batch)                 # symmetric bit for bit
        assert torch.equal(model.distance(a, b), batch)                 # and repeatable
        zero = model.distance(a, a)                                     # masked pairs included
        G.sync()
        assert (zero == 0.0).all() and (batch > 0).all()


def test_the_other_storage_build_gives_the_same_bits(model, tmp_path):
    """ONE child process in the other storage format (bf16 parent -> libhedit_hip_f16.so, and the reverse)"""
    other = "bf16" if _lib.STORAGE == "f16" else "f16"
    out = tmp_path / "child.npz"
    env = dict(os.environ, HEDIT_STORAGE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "sqlpips_child.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    c = np.load(out)
    assert int(c["is_f16"][0]) == (1 if other == "f16" else 0)
    for H, W, n in SC.CASES:
        a, b = SC.pairs(H, W, n)
        mine = model.distance(a.to(G.dev()), b.to(G.dev()))
        G.sync()
        assert np.array_equal(mine.cpu().numpy(), c[f"d{H}x{W}"]), (H, W)


def test_evaluator_end_to_end_with_standin_weights(model, tmp_path):
    from PIL import Image
    from evaluation import evaluation as EV
    d = tmp_path / "data" / "annotation_images" / "0_x"
    out = tmp_path / "res" / "0_x"
    d.mkdir(parents=True)
    out.mkdir(parents=True)
    mapping, images = {}, {}
    for i, name in enumerate(("a.png", "b.png")):
        s8, t8 = SR.uint8_pair(64, 64, 70 + i)
        Image.fromarray(s8).save(d / name)
        Image.fromarray(t8).save(out / name)
        images[f"00{i}"] = (s8, t8)
        mapping[f"00{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a bench",
                                 editing_type_id="0", mask=[64 * 16, 64 * 24])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    res = tmp_path / "results.csv"
    metrics = ["lpips", "lpips_unedit_part", "lpips_edit_part"]
    argv = ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "h_edit",
            "--tgt_folders", str(tmp_path / "res"), "--result_path", str(res), "--metrics"] + metrics
    assert EV.main(argv + ["--device", "cuda"], lpips=model) == 2
    rows = list(csv.reader(open(res)))
    assert rows[0] == ["file_id"] + [f"h_edit|{m}" for m in metrics] and [r[0] for r in rows[1:]] == ["000", "001"]
    mask = EV.mask_decode([64 * 16, 64 * 24], (64, 64))[:, :, None].repeat(3, axis=2)
    for r in rows[1:]:
        s8, t8 = images[r[0]]
        want = [model.score(s8, t8), model.score(s8, t8, 1 - mask, 1 - mask), model.score(s8, t8, mask, mask)]
        vals = [float(v) for v in r[1:]]
        print(f"[evaluator] {r[0]}: {vals}")
        assert vals == want and all(v > 0 for v in vals) and len(set(vals)) == 3
    assert model.scores([(s8, t8), (s8, t8, 1 - mask, 1 - mask), (s8, t8, mask, mask)]) == want      # one call, the same bits
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.main(argv + ["--device", "cpu"], lpips=model)
    with pytest.raises(NotImplementedError, match=r"torchmetrics LPIPS \(SqueezeNet\) weights"):
        EV.main(argv + ["--device", "cuda"])


def test_errors_are_reported_before_anything_is_launched(model):
    a, b = SC.pairs(36, 52, 3)
    a, b = a.to(G.dev()), b.to(G.dev())
    ok = model.distance(a, b).clone()
    n0 = model.calls
    with pytest.raises(ValueError, match="at least 32 x 32"):
        model.distance(a[:, :, :31], b[:, :, :31])
    with pytest.raises(ValueError, match="outside"):
        model.distance(a[:0], b[:0])
    with pytest.raises(ValueError, match="one shape"):
        model.distance(a, b[:2])
    with pytest.raises(RuntimeError, match="HIP executor only"):
        model.distance(a.cpu(), b.cpu())
    assert model.calls == n0
    lib, h = _lib.lib(), model._h
    N, H, W = 3, 36, 52
    out = torch.full((MAX_BATCH + 1,), -7.0, device=G.dev())
    need = lib.hedit_sqlpips_workspace_bytes(h, N, H, W)
    assert need > 0 and lib.hedit_sqlpips_workspace_bytes(h, 0, H, W) == 0 and lib.hedit_sqlpips_workspace_bytes(h, MAX_BATCH + 1, H, W) == 0
    assert lib.hedit_sqlpips_workspace_bytes(h, N, 31, W) == 0 and lib.hedit_sqlpips_workspace_bytes(h, N, 32, 33) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=G.dev())

    def call(hh=h, N=N, H=H, x=a, y=b, o=out, w=ws, nbytes=need):
        return lib.hedit_sqlpips_distance(hh, _lib.ptr(x), _lib.ptr(y), N, H, W, _lib.ptr(o), _lib.ptr(w), nbytes, _lib.cur_stream())

    raw = C.c_void_p()                                                      # created, nothing loaded: not finalized
    assert lib.hedit_sqlpips_create(C.byref(raw)) == 0
    try:
        assert lib.hedit_sqlpips_missing(raw) == lib.hedit_sqlpips_num_params(raw) == 2 + 6 * 8 + 7
        assert lib.hedit_sqlpips_finalize(raw, _lib.cur_stream()) == -3 and "unloaded parameters" in lib.hedit_last_error().decode()
        assert call(hh=raw) == -3 and "hedit_sqlpips_finalize" in lib.hedit_last_error().decode()
        assert lib.hedit_sqlpips_load(raw, b"features.5.weight", _lib.ptr(a), 4, _lib.cur_stream()) == -1
        assert "unknown SqueezeNet-LPIPS parameter" in lib.hedit_last_error().decode()
    finally:
        lib.hedit_sqlpips_destroy(raw)
    for kw, msg in ((dict(H=31), "at least 32"), (dict(N=0), "1 <= N <= 64"), (dict(N=MAX_BATCH + 1), "1 <= N <= 64"),
                    (dict(nbytes=need // 2), "workspace too small"), (dict(w=None), "null workspace"), (dict(x=None), "null"), (dict(o=None), "null")):
        rc = call(**kw)                                                     # the message is that of the LAST failed call: read it right away
        assert rc == -1 and msg in lib.hedit_last_error().decode(), (kw, rc, msg, lib.hedit_last_error())
    G.sync()
    assert (out == -7.0).all()                                              # nothing ran
    assert call() == 0
    G.sync()
    assert torch.equal(out[:N], ok) and (out[N:] == -7.0).all()
