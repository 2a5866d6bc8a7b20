"""Host side of SqueezeNet-LPIPS (hedit/lpips_score.py, csrc/sqlpips.hip; no GPU): the torch restatement the GPU tests use
as their reference (tests/helpers/sqlpips_ref.py, PARITY UNPINNED) has the tap sizes of the published network, the loader's
three key spellings, its refusals, the reference's preprocessing, the evaluator's routing and the declared exports."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-edit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import sqlpips_ref as SR  # noqa: E402
from hedit import lpips_score as LS  # noqa: E402

# torchvision index -> the slice of the lpips package's squeezenet that holds it (slice1 = features 0-1, slice2 = 2-4,
# slice3 = 5-7, slice4 = 8-9, slice5 = 10, slice6 = 11, slice7 = 12)
SLICE_OF = {0: 1, 3: 2, 4: 2, 6: 3, 7: 3, 9: 4, 10: 5, 11: 6, 12: 7}
TAP_SIZES = {(34, 46): [(16, 22), (8, 11), (4, 5), (2, 2)], (36, 52): [(17, 25), (8, 12), (4, 6), (2, 3)],
             (64, 64): [(31, 31), (15, 15), (7, 7), (3, 3)]}


@pytest.fixture(scope="module")
def net():
    return LS.SqueezeLpipsNet().init_random(5)


def test_tap_shapes_of_the_restatement(net):
    for (H, W), sizes in TAP_SIZES.items():
        with torch.no_grad():
            taps = SR.taps(net.params, torch.zeros(1, 3, H, W), torch.float32)
        want = sizes[:3] + [sizes[3]] * 4
        assert [tuple(t.shape) for t in taps] == [(1, c) + s for c, s in zip(LS.TAP_CHANNELS, want)], (H, W)
    assert sum(int(np.prod(s)) for k, s in net.param_shapes.items() if k.startswith("features.")) == 722496
    assert sum(1 for k in net.param_shapes if k.startswith("lin")) == 7


def test_identical_images_give_zero_and_different_ones_do_not(net):
    a8, b8 = SR.uint8_pair(34, 46, 1)
    a, b = LS.preprocess_pair(a8, b8)
    assert float(SR.distance(net.params, a[None], a[None])[0]) == 0.0
    d = float(SR.distance(net.params, a[None], b[None])[0])
    assert d > 0 and abs(float(SR.distance(net.params, b[None], a[None])[0]) - d) < 1e-15
    d32 = float(SR.distance(net.params, a[None], b[None], torch.float32)[0])
    assert abs(d32 - d) < 1e-5 * d
    assert all(float(v.min()) >= 0 for k, v in net.params.items() if k.startswith("lin"))


def _spellings(params):
    tv, lp, tm = {}, {}, {}
    for k, v in params.items():
        if k.startswith("lin"):
            tv[k] = lp[k] = tm[k] = v
            lp["lins." + k[3:]] = v                      # the duplicate listing of newer lpips versions
            continue
        i, rest = re.match(r"features\.(\d+)\.(.+)", k).groups()
        tv[k] = v
        lp[f"net.slice{SLICE_OF[int(i)]}.{i}.{rest}"] = v
        tm[f"net.slices.{SLICE_OF[int(i)] - 1}.{i}.{rest}"] = v
    for d in (lp, tm):
        d["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
        d["scaling_layer.scale"] = torch.ones(1, 3, 1, 1)
    return tv, lp, tm


def test_three_spellings_load_to_identical_containers(net, tmp_path):
    for sd in _spellings(net.params):
        got = LS.SqueezeLpipsNet().load_state_dict(sd).state_dict()
        assert list(got) == list(net.param_shapes)
        assert all(torch.equal(got[k], net.params[k]) for k in got)
    # one full file, a directory with the backbone and the lin file, and a (backbone, lins) pair
    tv, lp, _ = _spellings(net.params)
    torch.save(lp, tmp_path / "full.pth")
    d = tmp_path / "two"
    d.mkdir()
    backbone = {k: v for k, v in tv.items() if k.startswith("features.")}
    backbone["classifier.1.weight"] = torch.zeros(4, 512, 1, 1)          # torchvision's state dict carries the classifier
    lins = {k: v for k, v in tv.items() if k.startswith("lin")}
    torch.save(backbone, d / "squeezenet1_1.pth")
    torch.save(lins, d / "squeeze_lins.pth")
    for w in (str(tmp_path / "full.pth"), str(d), (str(d / "squeezenet1_1.pth"), lins), tv):
        m = LS.NativeSqueezeLpips(w, device="cpu")
        assert all(torch.equal(m.net.params[k], net.params[k]) for k in net.param_shapes)
    with pytest.raises(FileNotFoundError, match="nothing is fetched"):
        LS.NativeSqueezeLpips(str(tmp_path / "absent.pth"), device="cpu")


def test_unknown_and_missing_names_are_reported(net):
    tv, lp, _ = _spellings(net.params)
    bad = dict(tv)
    del bad["features.9.expand3x3.bias"], bad["lin4.model.1.weight"]
    bad["net.slice9.extra.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as e:
        LS.SqueezeLpipsNet().load_state_dict(bad)
    msg = str(e.value)
    assert "features.9.expand3x3.bias" in msg and "lin4.model.1.weight" in msg and "net.slice9.extra.weight" in msg and "(2)" in msg and "(1)" in msg
    with pytest.raises(ValueError, match="features.3.squeeze.weight: expected shape"):
        LS.SqueezeLpipsNet().load_state_dict(dict(tv, **{"features.3.squeeze.weight": torch.zeros(16, 64)}))
    with pytest.raises(KeyError, match="second, different value"):
        LS.canonical_names(dict(lp, **{"features.0.bias": torch.ones(64) * 9}))


def test_preprocessing_is_the_references(net):
    a8, b8 = SR.uint8_pair(36, 52, 2)
    m = SR.upper_half_mask(36, 52)
    a, b = LS.preprocess_pair(a8, b8, m, None)
    want_a = torch.tensor((a8.astype(np.float32) / 255) * m.astype(np.float32)).permute(2, 0, 1) * 2 - 1
    want_b = torch.tensor(b8.astype(np.float32) / 255).permute(2, 0, 1) * 2 - 1
    assert a.dtype == torch.float32 and a.shape == (3, 36, 52) and torch.equal(a, want_a) and torch.equal(b, want_b)
    assert (a[:, :18] == -1).all() and float(a.max()) <= 1 and float(b.min()) >= -1
    from PIL import Image
    pa, _ = LS.preprocess_pair(Image.fromarray(a8), Image.fromarray(b8), m, m)
    assert torch.equal(pa, a)


def test_there_is_no_cpu_path():
    m = LS.NativeSqueezeLpips(device="cpu")
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="HIP executor only"):
        m.distance(x, x)
    with pytest.raises(RuntimeError, match="HIP executor only"):
        m.score(np.zeros((32, 32, 3), dtype=np.uint8), np.zeros((32, 32, 3), dtype=np.uint8))


class FakeLpips:
    def __init__(self):
        self.seen = []

    def score(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        self.seen.append((np.array(img_pred), np.array(img_gt), mask_pred, mask_gt))
        return 0.25


def test_evaluator_routes_images_and_masks():
    from PIL import Image
    from evaluation import evaluation as EV
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(40, 40, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, size=(40, 40, 3), dtype=np.uint8)
    mask = np.zeros((40, 40, 3))
    mask[4:9] = 1
    fake = FakeLpips()
    mc = EV.MetricsCalculator("cuda", lpips=fake)
    args = (Image.fromarray(src), Image.fromarray(tgt), mask, mask, "a cat", "a dog")
    for m in ("lpips", "lpips_unedit_part", "lpips_edit_part"):
        assert EV.calculate_metric(mc, m, *args) == 0.25
    whole, unedit, edit = fake.seen
    assert all(np.array_equal(s[0], src) and np.array_equal(s[1], tgt) for s in fake.seen)
    assert whole[2] is None and whole[3] is None
    assert np.array_equal(unedit[2], 1 - mask) and np.array_equal(unedit[3], 1 - mask)
    assert np.array_equal(edit[2], mask) and np.array_equal(edit[3], mask)
    # the "nan" rules of the pixel metrics
    zero, one = np.zeros_like(mask), np.ones_like(mask)
    assert EV.calculate_metric(mc, "lpips_edit_part", args[0], args[1], mask, zero, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "lpips_edit_part", args[0], args[1], zero, mask, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "lpips_unedit_part", args[0], args[1], one, mask, "a", "b") == "nan"
    assert EV.calculate_metric(mc, "lpips_unedit_part", args[0], args[1], mask, one, "a", "b") == "nan"
    assert len(fake.seen) == 3
    assert mc.calculate_lpips(args[0], args[1], mask, None) == 0.25 and fake.seen[-1][3] is None
    # the pixel metrics are untouched, the other network metrics stay refused, and without a scorer lpips is refused as before
    assert EV.calculate_metric(EV.MetricsCalculator(), "mse", *args) > 0
    for m in ("local_clip", "structure_distance", "structure_distance_unedit_part", "clip_similarity_source_image"):
        with pytest.raises(NotImplementedError):
            EV.calculate_metric(mc, m, *args)
    with pytest.raises(ValueError, match="unknown metric"):
        EV.calculate_metric(mc, "lpips_whole", *args)
    for m in ("lpips", "lpips_unedit_part", "lpips_edit_part"):
        with pytest.raises(NotImplementedError, match=r"needs torchmetrics LPIPS \(SqueezeNet\) weights"):
            EV.calculate_metric(EV.MetricsCalculator(), m, *args)
    with pytest.raises(NotImplementedError, match="lpips_path"):
        EV.MetricsCalculator().calculate_lpips(args[0], args[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.MetricsCalculator("cpu", lpips=fake)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EV.load_lpips("/nonexistent", "cpu")


def test_parser_defaults():
    from evaluation import evaluation as EV
    ns = EV.build_parser().parse_args([])
    assert ns.lpips_path is None and ns.clip_path is None and ns.device == "cpu"
    assert ns.metrics == ["psnr_unedit_part", "mse_unedit_part", "ssim_unedit_part"]
    assert EV.build_parser().parse_args(["--lpips_path", "w.pth"]).lpips_path == "w.pth"


def test_new_exports_are_declared():
    from hedit import _lib
    hdr = open(os.path.join(ROOT, "include", "hedit.h")).read()
    declared = set(re.findall(r"\b(hedit_sqlpips_[a-z0-9_]+)\s*\(", hdr))
    want = {"hedit_sqlpips_" + s for s in ("create", "destroy", "num_params", "param_name", "param_shape", "load", "missing", "finalize",
                                           "workspace_bytes", "distance")}
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith("hedit_sqlpips_")}
    assert LS.MAX_BATCH == int(re.search(r"#define HEDIT_SQLPIPS_MAX_BATCH (\d+)", hdr).group(1)) >= 64
    src = open(os.path.join(ROOT, "h-edit_amd", "csrc", "sqlpips.hip")).read()
    table = re.search(r"FIRE\[NFIRE\]\[4\] = (\{.*?\});", src, re.S).group(1)
    assert tuple(tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{(\d+, \d+, \d+, \d+)\}", table)) == LS.FIRES
