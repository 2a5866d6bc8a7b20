"""-m gpu: the native DINO ViT key extractor and the key self-similarity distance (hedit_dino_* of csrc/dino.hip on the shared encoder
kernels and block forward of csrc/encoder.hip / encoder.h, behind
hedit.dino_score.NativeDinoStructure) and the evaluator's structure_distance columns, on seeded stand-in weights with chosen
scales (DinoNet.init_random), against the fp64 torch restatement tests/helpers/dino_ref.py run on the CPU.  PARITY UNPINNED
against the published network: no DINO code or weights exist offline and the reference tree holds no vector for this metric;
what is checked is the native executor against the restatement (which tests/test_host_dino.py pins to an independent build
from torch.nn.TransformerEncoderLayer and to F.interpolate).

Limits.  A distance: |native - ref| <= LIM |ref| + 1e-9; keys: max|native - ref| <= KEY_LIM max|ref|.  Each is 16 x the
largest error of torch's own fp32 restatement against the fp64 one on exactly the parity inputs, rounded up to one digit: a
three-term split-bf16 product drops the lo.lo term and the fixed chunk order differs from torch's, so a few times fp32's
error is expected, and 16 x stays far below the smallest wrong-variant effect (6.5e-4, tests/test_host_dino.py).
  fp32 against fp64, distance, whole / upper half masked (CPU):
    26 tokens 5.4e-7 / 2.0e-6;  145 tokens 6.7e-7 / 8.2e-8;  785 tokens 5.7e-7 / 4.8e-7;  patch 16 5.4e-7 / 9.8e-8;
    W 768 1.6e-7                                  -> largest 2.0e-6, x 16 = 3.2e-5  -> LIM = 4e-5
  fp32 against fp64, keys: 145 tokens 8.7e-7;  785 tokens 3.8e-6;  key_layer 0 1.1e-6;  one layer 1.4e-6
                                                  -> largest 3.8e-6, x 16 = 6.0e-5  -> KEY_LIM = 7e-5
Batch, argument-order, repeat, grid and storage-format comparisons are bit for bit.

MEASURED (MI355X, bfloat16 build; every parity test prints its figures with -s before it asserts):
  distance, |native - ref| / |ref|, whole / upper half masked:
    26 tokens 1.6e-5 / 1.8e-5;  145 tokens 4.1e-7 / 7.4e-6;  785 tokens 7.3e-6 / 5.4e-6;  patch 16, W 384 5.1e-6 / 2.4e-6;
    W 768, 785 tokens 2.6e-7;  key_layer 0 of three layers 1.7e-6;  one layer 8.8e-7
  keys, max|native - ref| / max|ref|: 145 tokens 1.1e-5;  785 tokens 1.1e-5;  key_layer 0 7.5e-6;  one layer 6.9e-6
  (the split-bf16 operands of the linear layers carry 16 mantissa bits: that is the 1e-5 of the keys)
Wall time of the file: 6.5 s inside pytest, of which the child process in the other storage build 2.3 s.
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
from helpers import dino_child as DC  # noqa: E402
from helpers import dino_ref as DR  # noqa: E402
from hedit import _lib  # noqa: E402
from hedit.dino_score import MAX_PAIRS, DinoNet, NativeDinoStructure  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_models = {}


def model(name):
    """the native scorer of a parity case, created once"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if name not in _models:
        _models[name] = NativeDinoStructure(DR.net_of(name), device=G.dev())
    return _models[name]


def _within(native, ref, what):
    native, ref = float(native), float(ref)
    err = abs(native - ref)
    print(f"[dino parity] {what}: native {native:.9e} ref {ref:.9e} |diff| {err:.3e} = {err / max(abs(ref), 1e-300):.3e} relative")
    assert err <= DR.LIM * abs(ref) + 1e-9, (what, native, ref)


def _keys_within(native, ref, what):
    err = ((native.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"[dino keys] {what}: max|native - ref| / max|ref| = {err:.3e} (max|ref| {ref.abs().max().item():.3e})")
    assert native.shape == ref.shape and err <= DR.KEY_LIM, (what, err)


@pytest.mark.parametrize("name", ["t26", "t145", "t785", "p16"])
def test_distance_parity_with_the_fp64_restatement(name):
    """26 tokens: one ragged key tile, every Gram tile ragged; 145: several key tiles and a ragged tail; 785: production's
    tile counts and resize ratio; patch 16 at W 384 without a resize.  Each whole and with the upper half masked."""
    m = model(name)
    _, _, k, patch, R, _, _ = DR.CASES[name]
    a, b = DR.parity_inputs(name)
    ref = DR.distance(m.net.params, a, b, patch, R, k)
    got = m.distance(a.to(G.dev()), b.to(G.dev())).cpu()
    for i, tag in enumerate(("whole", "upper half masked")):
        _within(got[i], ref[i], f"{name} {tag}")
    assert float(ref[0]) > 0 and float(ref[1]) > 0 and float(ref[0]) != float(ref[1])


def test_distance_parity_at_vit_b_width():
    """W 768, 12 heads, 785 tokens from 512 x 512: production's GEMM shapes, one pair"""
    m = model("vitb")
    _, _, k, patch, R, _, _ = DR.CASES["vitb"]
    a, b = DR.parity_inputs("vitb")
    a, b = a[:1], b[:1]
    ref = DR.distance(m.net.params, a, b, patch, R, k)
    got = m.distance(a.to(G.dev()), b.to(G.dev())).cpu()
    _within(got[0], ref[0], "vitb whole")


@pytest.mark.parametrize("name", ["t145", "t785"])
def test_keys_parity(name):
    m = model(name)
    _, _, k, patch, R, _, _ = DR.CASES[name]
    a, _ = DR.parity_inputs(name)
    _keys_within(m.keys(a.to(G.dev())).cpu(), DR.keys(m.net.params, a, patch, R, k), name)


@pytest.mark.parametrize("layers,k,seed", [(3, 0, 26), (1, 0, 27)])
def test_keys_straight_from_the_embedding(layers, k, seed):
    """key_layer 0: no attention runs and workspace_bytes must still suffice; and the one-layer network"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    net = DinoNet(128, layers, 8, 96, k).init_random(seed)
    m = NativeDinoStructure(net, device=G.dev())
    a, b = DR.parity_inputs("t145")
    assert [n for n in net.params if n.startswith("blocks.")] == [f"blocks.0.{s}" for s in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias")]
    _keys_within(m.keys(a.to(G.dev())).cpu(), DR.keys(net.params, a, 8, 96, k), f"layers {layers} key_layer {k}")
    _within(m.distance(a.to(G.dev()), b.to(G.dev())).cpu()[0], DR.distance(net.params, a, b, 8, 96, k)[0], f"layers {layers} key_layer {k}")


@pytest.mark.parametrize("N", [3, 5])
def test_a_batch_gives_the_bits_of_single_calls(N):
    for name in ("t145", "t785"):
        m = model(name)
        a, b = DC.pairs(name, N, seed0=500 + N)
        a, b = a.to(G.dev()), b.to(G.dev())
        n0 = m.calls
        batch = m.distance(a, b)
        assert m.calls == n0 + 1
        single = torch.cat([m.distance(a[i:i + 1], b[i:i + 1]) for i in range(N)])
        G.sync()
        assert torch.equal(batch, single), (name, batch, single)
        assert torch.equal(m.distance(b, a), batch)                 # symmetric bit for bit
        assert torch.equal(m.distance(a, b), batch)                 # and repeatable
        zero = m.distance(a, a)                                     # masked pairs included
        G.sync()
        assert (zero == 0.0).all() and (batch > 0).all(), (name, zero, batch)
        kb = m.keys(a)
        assert torch.equal(kb, torch.cat([m.keys(a[i:i + 1]) for i in range(N)]))


def test_the_attention_grid_does_not_change_the_keys():
    m = model("t785")
    a, _ = DC.pairs("t785", 2)
    a = a.to(G.dev())
    lib = _lib.lib()
    want = m.keys(a).clone()
    try:
        for s in (1, 2):
            _lib.check(lib.hedit_dino_set_slices(m._h, s))
            assert torch.equal(m.keys(a), want), s
    finally:
        _lib.check(lib.hedit_dino_set_slices(m._h, 0))
    assert torch.equal(m.keys(a), want)
    assert lib.hedit_dino_set_slices(m._h, -1) == -1


def test_full_vit_b8_depth_properties():
    """12 / 11 at W 768, N = 2, stand-in weights: properties only, no fp64 reference"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m = NativeDinoStructure(device=G.dev(), seed=5)
    assert (m.net.width, m.net.layers, m.net.heads, m.net.patch, m.net.key_layer, m.net.tokens) == (768, 12, 12, 8, 11, 785)
    a, b = DC.pairs("t785", 2, seed0=900)
    a, b = a.to(G.dev()), b.to(G.dev())
    batch = m.distance(a, b)
    single = torch.cat([m.distance(a[i:i + 1], b[i:i + 1]) for i in range(2)])
    zero = m.distance(b, b)
    G.sync()
    print(f"[dino full depth] distances {batch.tolist()}")
    assert torch.equal(batch, single) and (zero == 0.0).all() and torch.isfinite(batch).all() and (batch > 0).all()


def test_the_other_storage_build_gives_the_same_bits(tmp_path):
    """ONE child process in the other storage format (bf16 parent -> libhedit_hip_f16.so, and the reverse)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    other = "bf16" if _lib.STORAGE == "f16" else "f16"
    out = tmp_path / "child.npz"
    env = dict(os.environ, HEDIT_STORAGE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "dino_child.py"), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    c = np.load(out)
    assert int(c["is_f16"][0]) == (1 if other == "f16" else 0)
    for name, n in DC.CASES:
        a, b = DC.pairs(name, n)
        mine = model(name).distance(a.to(G.dev()), b.to(G.dev()))
        keys = model(name).keys(a[:2].to(G.dev()))
        G.sync()
        assert np.array_equal(mine.cpu().numpy(), c[f"d_{name}"]), name
        assert np.array_equal(keys.cpu().numpy(), c[f"k_{name}"]), name


def test_evaluator_end_to_end_with_a_state_dict_file(tmp_path):
    from PIL import Image
    from evaluation import evaluation as EV
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    net = DR.net_of("t26")
    sd = net.state_dict()
    sd["norm.weight"], sd["norm.bias"] = torch.ones(128), torch.zeros(128)       # names the executor does not use
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.save(sd, wdir / "dino_tiny.pth")
    d = tmp_path / "data" / "annotation_images" / "0_x"
    out = tmp_path / "res" / "0_x"
    d.mkdir(parents=True)
    out.mkdir(parents=True)
    mapping, images = {}, {}
    for i, name in enumerate(("a.png", "b.png")):
        s8, t8 = DR.uint8_pair(64, 70 + i)
        Image.fromarray(s8).save(d / name)
        Image.fromarray(t8).save(out / name)
        images[f"00{i}"] = (s8, t8)
        mapping[f"00{i}"] = dict(image_path=f"0_x/{name}", original_prompt="a [cat] on a bench", editing_prompt="a [dog] on a bench",
                                 editing_type_id="0", mask=[64 * 16, 64 * 24])
    mf = tmp_path / "data" / "mapping_file.json"
    json.dump(mapping, open(mf, "w"))
    res = tmp_path / "results.csv"
    metrics = ["structure_distance", "structure_distance_unedit_part", "structure_distance_edit_part"]
    argv = ["--annotation_mapping_file", str(mf), "--src_image_folder", str(tmp_path / "data" / "annotation_images"), "--tgt_methods", "h_edit",
            "--tgt_folders", str(tmp_path / "res"), "--result_path", str(res), "--metrics"] + metrics
    with pytest.raises(ValueError, match="positional-embedding interpolation is out of scope"):
        EV.main(argv + ["--dino_path", str(wdir), "--device", "cuda"])             # 26 rows do not fit the default 224
    with pytest.raises(ValueError, match="key_layer"):
        EV.load_dino(str(wdir), "cuda", 40)                                         # block 11 of a 3-block network
    model = NativeDinoStructure(str(wdir / "dino_tiny.pth"), device=G.dev(), resolution=40, key_layer=2)
    assert model.net.ignored == ["norm.bias", "norm.weight"]
    assert EV.main(argv + ["--device", "cuda"], dino=model) == 2
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
        EV.main(argv + ["--device", "cpu"], dino=model)
    with pytest.raises(NotImplementedError, match="DINO ViT-B/8 weights"):
        EV.main(argv + ["--device", "cuda"])


def test_errors_are_reported_before_anything_is_launched():
    m = model("t145")
    a, b = DC.pairs("t145", 3)
    a, b = a.to(G.dev()), b.to(G.dev())
    ok = m.distance(a, b).clone()
    n0 = m.calls
    with pytest.raises(ValueError, match="non-square"):
        m.distance(a[:, :, :100], b[:, :, :100])
    with pytest.raises(ValueError, match="outside"):
        m.distance(a[:, :, :4, :4], b[:, :, :4, :4])
    with pytest.raises(ValueError, match="empty"):
        m.distance(a[:0], b[:0])
    with pytest.raises(ValueError, match="one shape"):
        m.distance(a, b[:2])
    with pytest.raises(RuntimeError, match="HIP executor only"):
        m.distance(a.cpu(), b.cpu())
    assert m.calls == n0
    lib, h = _lib.lib(), m._h
    N, S = 3, 128
    # creation refuses, before any allocation
    for cfg, msg in (((128, 3, 4, 8, 96, 2), "head dimension must be 64"), ((128, 3, 2, 8, 100, 2), "multiple of patch_size"),
                     ((128, 3, 2, 8, 96, 3), "key_layer"), ((128, 3, 2, 8, 96, -1), "key_layer"), ((128, 3, 2, 8, 264, 2), "at most 1025 tokens")):
        raw = C.c_void_p()
        c = _lib.DinoCfg(*cfg)
        assert lib.hedit_dino_create(C.byref(c), C.byref(raw)) == -1 and msg in lib.hedit_last_error().decode(), (cfg, lib.hedit_last_error())
        assert raw.value is None
    out = torch.full((MAX_PAIRS + 1,), -7.0, device=G.dev())
    kout = torch.full((2, 145, 128), -7.0, device=G.dev())
    need = lib.hedit_dino_workspace_bytes(h, N, S)
    assert need > 0 and lib.hedit_dino_workspace_bytes(h, 0, S) == 0 and lib.hedit_dino_workspace_bytes(h, MAX_PAIRS + 1, S) == 0
    assert lib.hedit_dino_workspace_bytes(h, N, 7) == 0 and lib.hedit_dino_workspace_bytes(h, N, 4097) == 0 and lib.hedit_dino_workspace_bytes(h, N, 8) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=G.dev())

    def call(hh=h, N=N, S=S, x=a, y=b, o=out, w=ws, nbytes=need):
        return lib.hedit_dino_structure_distance(hh, _lib.ptr(x), _lib.ptr(y), N, S, _lib.ptr(o), _lib.ptr(w), nbytes, _lib.cur_stream())

    def kcall(hh=h, B=2, S=S, x=a, o=kout, w=ws, nbytes=need):
        return lib.hedit_dino_keys(hh, _lib.ptr(x), B, S, _lib.ptr(o), _lib.ptr(w), nbytes, _lib.cur_stream())

    raw = C.c_void_p()                                                      # created, nothing loaded: not finalized
    c = _lib.DinoCfg(128, 3, 2, 8, 96, 2)
    assert lib.hedit_dino_create(C.byref(c), C.byref(raw)) == 0
    try:
        assert lib.hedit_dino_missing(raw) == lib.hedit_dino_num_params(raw) == 4 + 2 * 12 + 4
        assert lib.hedit_dino_finalize(raw, _lib.cur_stream()) == -3 and "unloaded parameters" in lib.hedit_last_error().decode()
        assert call(hh=raw) == -3 and "hedit_dino_finalize" in lib.hedit_last_error().decode()
        assert kcall(hh=raw) == -3 and "hedit_dino_finalize" in lib.hedit_last_error().decode()
        assert lib.hedit_dino_load(raw, b"blocks.2.mlp.fc1.weight", _lib.ptr(a), 4, _lib.cur_stream()) == -1
        assert "unknown DINO ViT parameter" in lib.hedit_last_error().decode()
    finally:
        lib.hedit_dino_destroy(raw)
    for kw, msg in ((dict(S=7), "[patch_size, 4096]"), (dict(S=4097), "[patch_size, 4096]"), (dict(N=0), "1 <= N <= 64"),
                    (dict(N=MAX_PAIRS + 1), "1 <= N <= 64"), (dict(nbytes=need // 2), "workspace too small (need "), (dict(w=None), "null workspace"),
                    (dict(x=None), "null"), (dict(o=None), "null")):
        rc = call(**kw)                                                     # the message is that of the LAST failed call: read it right away
        assert rc == -1 and msg in lib.hedit_last_error().decode(), (kw, rc, msg, lib.hedit_last_error())
    for kw, msg in ((dict(S=7), "[patch_size, 4096]"), (dict(B=0), "1 <= B <= 128"), (dict(B=2 * MAX_PAIRS + 1), "1 <= B <= 128"),
                    (dict(nbytes=1024), "workspace too small (need "), (dict(w=None), "null workspace"), (dict(x=None), "null")):
        rc = kcall(**kw)
        assert rc == -1 and msg in lib.hedit_last_error().decode(), (kw, rc, msg, lib.hedit_last_error())
    G.sync()
    assert (out == -7.0).all() and (kout == -7.0).all()                     # nothing ran
    assert call() == 0 and kcall() == 0
    G.sync()
    assert torch.equal(out[:N], ok) and (out[N:] == -7.0).all() and torch.equal(kout, m.keys(a[:2]))
