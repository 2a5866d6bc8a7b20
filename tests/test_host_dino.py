"""Host side of the Structure Distance (hedit/dino_score.py, csrc/dino.hip; no GPU): the fp64 torch restatement the GPU tests
use as their reference (tests/helpers/dino_ref.py, PARITY UNPINNED against the published network) against an independent
build from torch.nn.TransformerEncoderLayer, its resize against F.interpolate, that the GPU tests' limit can see every wrong
variant, ``DinoNet.from_state_dict``, the evaluator's routing, the parser and the declared exports.

The limit bites.  LIM = 4e-5 (tests/test_gpu_dino.py derives it), so a wrong variant has to move the fp64 distance by
>= 4e-4 relative.  Measured on the parity inputs (whole / upper half masked), smallest figure over the cases it applies to:
QuickGELU 1.4e-3, LayerNorm eps 1e-5 6.5e-4, input / 255 0.9999, antialiased resize 3.0e-2, keys of block k - 1 2.3e-1,
``n_i n_j + eps`` for ``clamp`` 1.6e-3.  tanh-GELU does NOT reach 10 x LIM in any case: 4.4e-6 ... 2.3e-4 (largest: 26 tokens,
whole image), and raising the MLP branch fourfold did not change that (1.1e-5 ... 2.5e-4) -- tanh-GELU is within 5e-4 of the
exact one everywhere.  What is asserted for it is the weaker statement that it exceeds LIM itself in at least one case, so the
GPU parity test of that case fails on it.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import dino_ref as DR  # noqa: E402
from hedit import dino_score as DS  # noqa: E402

BITE_CASES = ("t26", "t145", "t785", "p16")          # the parity cases below ViT-B width (whose fp64 pass takes over a second)
_cache = {}


def _case(name):
    """(net, a, b, fp64 distance) of a parity case, computed once"""
    if name not in _cache:
        net = DR.net_of(name)
        a, b = DR.parity_inputs(name)
        _, _, k, patch, R, _, _ = DR.CASES[name]
        _cache[name] = (net, a, b, DR.distance(net.params, a, b, patch, R, k))
    return _cache[name]


def _moved(name, key_layer=None, **variant):
    net, a, b, ref = _case(name)
    _, _, k, patch, R, _, _ = DR.CASES[name]
    v = DR.distance(net.params, a, b, patch, R, k if key_layer is None else key_layer, **variant)
    return ((v - ref).abs() / ref).tolist()


def test_restatement_against_an_independent_build():
    """the same tiny network from torch.nn.TransformerEncoderLayer; the keys of the last block are norm1(x) @ W_k^T + b_k"""
    W, layers, patch, R = 128, 3, 8, 40
    net = DS.DinoNet(W, layers, patch, R).init_random(3)
    P = {k: v.double() for k, v in net.params.items()}
    a, _ = DR.parity_inputs("t26")
    x = DR.tokens(P, DR.preprocess(a.double(), R), patch)
    for i in range(layers - 1):
        lay = torch.nn.TransformerEncoderLayer(W, W // 64, 4 * W, dropout=0.0, activation="gelu", layer_norm_eps=1e-6, batch_first=True,
                                               norm_first=True, dtype=torch.float64)
        p = f"blocks.{i}."
        with torch.no_grad():
            for dst, src in ((lay.self_attn.in_proj_weight, "attn.qkv.weight"), (lay.self_attn.in_proj_bias, "attn.qkv.bias"),
                             (lay.self_attn.out_proj.weight, "attn.proj.weight"), (lay.self_attn.out_proj.bias, "attn.proj.bias"),
                             (lay.linear1.weight, "mlp.fc1.weight"), (lay.linear1.bias, "mlp.fc1.bias"), (lay.linear2.weight, "mlp.fc2.weight"),
                             (lay.linear2.bias, "mlp.fc2.bias"), (lay.norm1.weight, "norm1.weight"), (lay.norm1.bias, "norm1.bias"),
                             (lay.norm2.weight, "norm2.weight"), (lay.norm2.bias, "norm2.bias")):
                dst.copy_(P[p + src])
        x = lay.train(False)(x).detach()          # parameters require grad: the plain (not the fused) path
    p = f"blocks.{layers - 1}."
    want = F.layer_norm(x, (W,), P[p + "norm1.weight"], P[p + "norm1.bias"], 1e-6) @ P[p + "attn.qkv.weight"][W:2 * W].T + P[p + "attn.qkv.bias"][W:2 * W]
    got = DR.keys(net.params, a, patch, R, layers - 1)
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"[dino restatement] max|keys - independent| / max|keys| = {err:.3e}")
    assert got.shape == (2, 26, W) and err < 1e-12


def test_resize_is_bilinear_without_antialias():
    g = torch.Generator().manual_seed(1)
    for S, R in ((64, 40), (128, 96), (512, 224), (20, 48)):
        x = torch.rand(2, 3, S, S, generator=g, dtype=torch.float64) * 255
        want = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False, antialias=False)
        assert (DR.resize(x, R) - want).abs().max() < 1e-10, (S, R)
    x = torch.rand(1, 3, 40, 40, generator=g, dtype=torch.float64)
    assert DR.resize(x, 40) is x
    for name in ("t26", "t145", "t785"):
        m = _moved(name, antialias=True)
        print(f"[dino bite] {name} antialiased resize: {m}")
        assert min(m) > 10 * DR.LIM


def test_torch_fp32_is_within_the_limit():
    """the limit is 16 x the error of torch's own fp32 restatement (measured figures: tests/test_gpu_dino.py); here only that
    fp32 itself passes it with room, on whatever machine this runs"""
    for name in BITE_CASES:
        net, a, b, ref = _case(name)
        _, _, k, patch, R, _, _ = DR.CASES[name]
        f32 = DR.distance(net.params, a, b, patch, R, k, dtype=torch.float32).double()
        k64, k32 = DR.keys(net.params, a, patch, R, k), DR.keys(net.params, a, patch, R, k, dtype=torch.float32).double()
        rel, krel = ((f32 - ref).abs() / ref).tolist(), ((k32 - k64).abs().max() / k64.abs().max()).item()
        print(f"[dino fp32] {name}: distance {ref.tolist()} fp32 relative error {rel}, keys {krel:.3e}")
        assert max(rel) < DR.LIM / 4 and krel < DR.KEY_LIM / 4 and (ref > 0).all() and float(ref[0]) != float(ref[1])


@pytest.mark.parametrize("tag,variant", [("QuickGELU", dict(gelu="quick")), ("eps 1e-5", dict(eps=1e-5)), ("input / 255", dict(div255=True)),
                                         ("keys of block k - 1", dict(key_layer=1)), ("+ eps for clamp", dict(clamp=False))])
def test_the_limit_bites(tag, variant):
    for name in BITE_CASES:
        m = _moved(name, **variant)
        print(f"[dino bite] {name} {tag}: {m}")
        assert min(m) >= 10 * DR.LIM, (name, tag, m)


def test_tanh_gelu_is_seen_in_at_least_one_case():
    """see the module docstring: 10 x LIM is out of reach for tanh-GELU at any scaling tried; LIM itself is exceeded"""
    m = {name: _moved(name, gelu="tanh") for name in BITE_CASES}
    print(f"[dino bite] tanh-GELU: {m}")
    assert max(max(v) for v in m.values()) > 4 * DR.LIM


VARIANTS = {"dino_vits16": (384, 16), "dino_vits8": (384, 8), "dino_vitb16": (768, 16), "dino_vitb8": (768, 8)}


def _shape_only(W, patch, layers=12, res=224):
    sd = {k: torch.empty(s) for k, s in DS.dino_param_shapes(W, patch, res, layers - 1).items()}
    for k in DS._WHOLE[4:]:
        sd[f"blocks.{layers - 1}.{k}"] = torch.empty(DS.dino_param_shapes(W, patch, res, layers - 1)[f"blocks.0.{k}"]) if layers > 1 else torch.empty(1)
    sd["norm.weight"], sd["norm.bias"] = torch.empty(W), torch.empty(W)
    return sd


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_from_state_dict_infers_the_published_variants(name):
    W, patch = VARIANTS[name]
    net = DS.DinoNet.from_state_dict(_shape_only(W, patch))
    assert (net.width, net.layers, net.heads, net.patch, net.resolution, net.key_layer) == (W, 12, W // 64, patch, 224, 11)
    assert net.tokens == (224 // patch) ** 2 + 1
    assert net.ignored == sorted(["norm.weight", "norm.bias"] + [f"blocks.11.{k}" for k in DS._WHOLE[4:]])
    assert list(net.params) == list(DS.dino_param_shapes(W, patch, 224, 11))


def test_from_state_dict_refusals_and_key_layer():
    sd = _shape_only(128, 8, layers=3, res=40)
    with pytest.raises(ValueError, match="positional-embedding interpolation is out of scope"):
        DS.DinoNet.from_state_dict(sd, key_layer=2)                  # 26 rows, 224 / 8 needs 785
    with pytest.raises(ValueError, match="positional-embedding interpolation is out of scope"):
        DS.DinoNet.from_state_dict(sd, resolution=44, key_layer=2)
    with pytest.raises(ValueError, match="key_layer"):
        DS.DinoNet.from_state_dict(sd, resolution=40)                # the default 11 of a 3-block network
    net = DS.DinoNet.from_state_dict({"module." + k: v for k, v in sd.items()}, resolution=40, key_layer=1)
    assert net.layers == 3 and net.key_layer == 1 and "blocks.2.norm1.weight" in net.ignored and "blocks.1.mlp.fc1.weight" in net.ignored
    assert "blocks.1.attn.qkv.weight" in net.params and "blocks.1.attn.proj.weight" not in net.params
    del sd["blocks.0.mlp.fc1.bias"]
    with pytest.raises(KeyError, match="blocks.0.mlp.fc1.bias"):
        DS.DinoNet.from_state_dict(sd, resolution=40, key_layer=2)
    with pytest.raises(FileNotFoundError, match="nothing is fetched"):
        DS.read_weights("/nonexistent/dino.pth")


def test_read_weights_takes_a_file_or_a_directory_with_one_pth(tmp_path):
    sd = DR.net_of("t26").state_dict()
    torch.save(sd, tmp_path / "w.pth")
    assert set(DS.read_weights(str(tmp_path))) == set(DS.read_weights(str(tmp_path / "w.pth"))) == set(sd)
    torch.save(sd, tmp_path / "w2.pth")
    with pytest.raises(FileNotFoundError, match="exactly one .pth"):
        DS.read_weights(str(tmp_path))


class FakeScorer:
    def __init__(self):
        self.seen = []

    def score(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        self.seen.append((img_pred, img_gt, mask_pred, mask_gt))
        return 0.125


def test_evaluator_routing_with_a_fake_scorer():
    from evaluation import evaluation as EV
    g = np.random.default_rng(0)
    src, tgt = (g.integers(0, 256, (16, 16, 3)).astype(np.uint8) for _ in range(2))
    mask = np.zeros((16, 16, 3))
    mask[4:9] = 1
    zero, one = np.zeros_like(mask), np.ones_like(mask)
    fake = FakeScorer()
    mc = EV.MetricsCalculator("cuda", dino=fake)
    args = (src, tgt, mask, mask, "a", "b")
    assert [EV.calculate_metric(mc, m, *args) for m in ("structure_distance", "structure_distance_unedit_part", "structure_distance_edit_part")] == [0.125] * 3
    (a0, b0, ma0, mb0), (a1, b1, ma1, mb1), (a2, b2, ma2, mb2) = fake.seen
    for a, b in ((a0, b0), (a1, b1), (a2, b2)):
        assert a is src and b is tgt                                  # images untouched
    assert ma0 is None and mb0 is None
    assert np.array_equal(ma1, 1 - mask) and np.array_equal(mb1, 1 - mask) and np.array_equal(ma2, mask) and np.array_equal(mb2, mask)
    # the four "nan" rules of the reference's evaluation.py:58-62,83-87
    assert EV.calculate_metric(mc, "structure_distance_edit_part", src, tgt, zero, mask, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "structure_distance_edit_part", src, tgt, mask, zero, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "structure_distance_unedit_part", src, tgt, one, mask, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "structure_distance_unedit_part", src, tgt, mask, one, "a", "b") == "nan"
    assert len(fake.seen) == 3
    # the other metrics are as before
    assert EV.calculate_metric(EV.MetricsCalculator(), "mse", *args) > 0
    for m in ("local_clip", "lpips", "clip_similarity_source_image"):
        with pytest.raises(NotImplementedError):
            EV.calculate_metric(mc, m, *args)
    with pytest.raises(ValueError, match="unknown metric"):
        EV.calculate_metric(mc, "structure_distance_whole", *args)
    # without a scorer all three names are refused as before
    for m in ("structure_distance", "structure_distance_unedit_part", "structure_distance_edit_part"):
        with pytest.raises(NotImplementedError, match="DINO ViT-B/8 weights"):
            EV.calculate_metric(EV.MetricsCalculator(), m, *args)
    with pytest.raises(NotImplementedError, match="dino_path"):
        EV.MetricsCalculator().calculate_structure_distance(src, tgt)


def test_there_is_no_cpu_path(tmp_path):
    from evaluation import evaluation as EV
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.MetricsCalculator("cpu", dino=FakeScorer())
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.load_dino(str(tmp_path / "w.pth"), "cpu")
    s = DS.NativeDinoStructure(DR.net_of("t26"), device="cpu")
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.score(img, img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.distance(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_score_refuses_non_square_and_unequal_inputs_on_the_host():
    s = DS.NativeDinoStructure(DR.net_of("t26"), device="cpu")
    with pytest.raises(ValueError, match="non-square"):
        s.score(np.zeros((16, 24, 3), np.uint8), np.zeros((16, 24, 3), np.uint8))
    with pytest.raises(ValueError, match="shapes should be the same"):
        s.score(np.zeros((16, 16, 3), np.uint8), np.zeros((24, 24, 3), np.uint8))
    a, b = DS.preprocess_pair(np.full((8, 8, 3), 200, np.uint8), np.full((8, 8, 3), 100, np.uint8), None, np.full((8, 8, 3), 0.5))
    assert a.dtype == torch.float32 and a.shape == (3, 8, 8) and float(a.max()) == 200.0 and float(b.max()) == 50.0      # no / 255


def test_parser_defaults():
    from evaluation import evaluation as EV
    ns = EV.build_parser().parse_args([])
    assert ns.dino_path is None and ns.dino_resolution == 224 and ns.lpips_path is None and ns.clip_path is None and ns.device == "cpu"
    assert ns.metrics == ["psnr_unedit_part", "mse_unedit_part", "ssim_unedit_part"]
    assert EV.build_parser().parse_args(["--dino_path", "w.pth"]).dino_path == "w.pth"


def test_new_exports_are_declared():
    from hedit import _lib
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    declared = set(re.findall(r"\b(hedit_dino_[a-z0-9_]+)\s*\(", hdr))
    want = {"hedit_dino_" + s for s in ("create", "destroy", "num_params", "param_name", "param_shape", "load", "missing", "finalize", "set_slices",
                                        "workspace_bytes", "keys", "structure_distance")}
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith("hedit_dino_")}
    assert DS.MAX_PAIRS == int(re.search(r"#define HEDIT_DINO_MAX_PAIRS (\d+)", hdr).group(1)) == 64
    src = open(os.path.join(ROOT, "h-edit_amd", "csrc", "dino.hip")).read()
    assert DS.MAX_TOKENS == int(re.search(r"constexpr int LMAX = (\d+);", src).group(1)) >= 785
    assert [f[0] for f in _lib.DinoCfg._fields_] == re.search(r"typedef struct \{ int ([a-z_, ]+); \} hedit_dino_cfg;", hdr).group(1).split(", ")
