"""-m gpu: the images the editing drivers (h-edit_amd/main_*.py on the shared scaffolding of hedit/driver.py) write are
pinned to tests/golden/g25_driver_bits.json: per case the SHA-256 of every written image's decoded uint8 pixel array (shape
and bytes; pixels, not file bytes, so the PNG encoder does not matter), keyed by the file's base name (a time stamp in it replaced by ``T``).

The golden file was written on an MI355X by the drivers of the commit it names (`parent_commit`: the last one in which
every driver carried its own copy of the scaffolding), never by the code under test:
    python tests/test_gpu_driver_bits.py --write --parent <commit> --drivers DIR
runs that commit's Python tree from DIR (a copy of its h-edit_amd/) on the product library -- csrc/ is the same in both, so
there is one library -- every case twice, and writes the JSON.  A case whose two runs agree is recorded under "cases"; one
whose runs disagree goes under "unstable" with both sets of hashes, which only a case that draws random numbers (eta > 0) may
do.  Under pytest the drivers of this tree must reproduce every recorded hash.  torch.manual_seed(0) precedes each main().

Every case: --random_init --tiny --num_diffusion_steps 4.  The text drivers run on the three entries of
helpers.datasets.pie_dataset (at --batch 2: one lock-step pair and a group of one), main_demo.py on the two-entry yaml of
test_gpu_driver.py::test_demo_driver_batch_flag, main_edit.py on the two-entry json of test_style_driver_writes_edited_images.
"""
import hashlib
import importlib.util
import json
import os
import pathlib
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PRODUCT = os.path.join(ROOT, "h-edit_amd")
WRITE = __name__ == "__main__" and "--write" in sys.argv
DRIVERS = os.path.abspath(sys.argv[sys.argv.index("--drivers") + 1]) if WRITE else PRODUCT
sys.path.insert(0, HERE)
sys.path.insert(0, DRIVERS)
from helpers.datasets import pie_dataset  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "g25_driver_bits.json")

_D_P2P = ["--mode", "h_edit_D_p2p", "--eta", "0.0", "--implicit"]
# case -> (driver, dataset, flags, batch sizes)
CASES = {
    "p2p_D_implicit_k2": ("main_p2p", "pie", _D_P2P + ["--optimization_steps", "2"], (1, 2)),
    "p2p_default": ("main_p2p", "pie", [], (1,)),
    "p2p_R_implicit": ("main_p2p", "pie", ["--mode", "h_edit_R", "--implicit"], (1,)),
    "masactrl_D_k2": ("main_masactrl", "pie", ["--step", "1", "--layer", "2", "--optimization_steps", "2"], (1, 2)),
    "pnp_D": ("main_plugnplay", "pie", ["--mode", "h_edit_D_pnp", "--eta", "0.0", "--pnp_f_t", "0.6"], (1, 2)),
    "demo_D_implicit": ("main_demo", "demo", _D_P2P, (1, 2)),
    "style_default": ("main_edit", "style", [], (1, 2)),
    "baselines_ef": ("main_baselines", "pie", ["--mode", "ef"], (1,)),
    "baselines_pnp_inv_p2p": ("main_baselines", "pie", ["--mode", "pnp_inv_p2p", "--eta", "0.0"], (1, 2)),
    "baselines_pnp_inv_masactrl": ("main_baselines", "pie", ["--mode", "pnp_inv_masactrl", "--eta", "0.0"], (1,)),
    "baselines_np_pnp": ("main_baselines", "pie", ["--mode", "np_pnp", "--eta", "0.0"], (1,)),
    "nmg_p2p": ("main_nmg", "pie", ["--mode", "nmg_p2p"], (1,)),
    "nmg_pnp": ("main_nmg", "pie", ["--mode", "nmg_pnp"], (1,)),
    "nt_pnp": ("main_nt", "pie", ["--mode", "nt_pnp"], (1, 2)),
}
RUNS = [(name, b) for name, c in CASES.items() for b in c[3]]
DRAWS_RANDOM = ("p2p_default", "p2p_R_implicit", "style_default", "baselines_ef")       # the eta > 0 cases


def _picture(fx, fy, fz):
    y, x = np.mgrid[0:96, 0:128]
    return np.stack([fx(x, y) % 256, fy(x, y) % 256, fz(x, y) % 256], -1).astype(np.uint8)


def demo_dataset(tmp_path):
    import yaml
    from PIL import Image
    d = tmp_path / "demo"
    d.mkdir()
    Image.fromarray(_picture(lambda x, y: x * 3, lambda x, y: y * 5, lambda x, y: x + y)).save(d / "lizard.png")
    Image.fromarray(_picture(lambda x, y: x * 7, lambda x, y: y * 2, lambda x, y: x * y)).save(d / "cat.png")
    with open(d / "demo.yaml", "w") as f:
        yaml.safe_dump([dict(image="/lizard.png", source_prompt="a green lizard is sitting on a branch",
                             target_prompt="a brown lizard is sitting on a branch", blended_word="lizard lizard",
                             editing_instruction=""),
                        dict(image="/cat.png", source_prompt="a cat", target_prompt="a cat wearing a big hat", blended_word="",
                             editing_instruction="")], f)
    return ["--data_path", str(d)]


def style_dataset(tmp_path):
    from PIL import Image
    d = tmp_path / "demo"
    (d / "styles").mkdir(parents=True)
    data = {}
    for i, (src, tar, blend) in enumerate([("an orange van with surfboards on top", "an orange van with flowers on top",
                                            "surfboards flowers"),
                                           ("a round cake on a plate", "a square cake on a wooden plate", "")]):
        Image.fromarray(_picture(lambda x, y: x * (i + 2), lambda x, y: y * 3 + i * 40, lambda x, y: x + y)).save(d / f"{i:012d}.jpg")
        Image.fromarray(_picture(lambda x, y: x * y + i, lambda x, y: x * 7, lambda x, y: y * 5)).save(d / "styles" / f"s{i}.png")
        data[f"{i:012d}"] = dict(image_path=f"{i:012d}.jpg", original_prompt=src, editing_prompt=tar,
                                 editing_instruction="", blended_word=blend, style=f"styles/s{i}.png")
    with open(d / "demo.json", "w") as f:
        json.dump(data, f)
    return ["--dataset", str(d) + "/"]


DATASETS = {"pie": lambda t: ["--data_path", str(pie_dataset(t))], "demo": demo_dataset, "style": style_dataset}


def _driver(name):
    spec = importlib.util.spec_from_file_location("hedit_bits_" + name, os.path.join(DRIVERS, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sha(path):
    from PIL import Image
    a = np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def run_case(name, batch, tmp_path):
    """{base name of a written image: SHA-256 of its pixels}"""
    drv, dataset, flags, _ = CASES[name]
    argv = DATASETS[dataset](tmp_path) + ["--output_path", str(tmp_path / "out"), "--random_init", "--tiny",
                                         "--num_diffusion_steps", "4", "--batch", str(batch)] + flags
    torch.manual_seed(0)
    written = _driver(drv).main(argv)
    # (main_edit.py writes into <output_path>/<sub><file>, as the reference does: its base names carry the run's time stamp)
    out = {re.sub(r"_time_\d+_", "_time_T_", os.path.basename(p)): _sha(p) for p in written}
    assert len(out) == len(written) > 1
    return out


@pytest.mark.parametrize("name,batch", RUNS)
def test_driver_output_bits_match_the_parent_commit(tmp_path, name, batch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    doc = json.load(open(GOLDEN))
    key = f"{name}_b{batch}"
    assert key in doc["cases"] or (key in doc["unstable"] and name in DRAWS_RANDOM), key
    got = run_case(name, batch, tmp_path)
    for base, h in got.items():
        print(f"[driver bits] {key} {base}: {h[:12]}")
    if key in doc["cases"]:
        assert got == doc["cases"][key], (key, got, doc["cases"][key])


if __name__ == "__main__":
    if not WRITE or "--drivers" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_driver_bits.py --write --parent COMMIT --drivers DIR [--out FILE]")
    from hedit import _lib
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(DRIVERS, "hedit"), _lib.__file__
    _lib.LIB_PATH = os.path.join(PRODUCT, "hedit", os.path.basename(_lib.LIB_PATH))       # the product library
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else "unknown"
    doc = dict(parent_commit=parent, cases={}, unstable={})
    for name, batch in RUNS:
        with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
            a, b = run_case(name, batch, pathlib.Path(t1)), run_case(name, batch, pathlib.Path(t2))
        key = f"{name}_b{batch}"
        if a == b:
            doc["cases"][key] = a
        else:
            assert name in DRAWS_RANDOM, f"{key} draws no random numbers and its two runs disagree: {a} {b}"
            doc["unstable"][key] = [a, b]
        print(key, "stable" if a == b else "UNSTABLE", flush=True)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from the drivers of", DRIVERS, "on", _lib.LIB_PATH)
