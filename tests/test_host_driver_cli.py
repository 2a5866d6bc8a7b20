"""The command line of every editing driver is pinned to tests/golden/g25_driver_cli.json: per driver the namespace
``vars(build_parser().parse_args([]))`` of the commit the file names (`parent_commit`: the last one in which every driver
typed out its own argparse block), written from that commit's files and never by the parsers under test, which now take the
shared flags from hedit/driver.py.  main_edit_face_ef.py has no parser of its own: it runs main_edit_face.py's."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "g25_driver_cli.json")) as f:
    GOLDEN = json.load(f)["drivers"]


def _driver(name):
    spec = importlib.util.spec_from_file_location("hedit_cli_" + name, os.path.join(ROOT, "h-edit_amd", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_driver_with_a_parser_is_pinned():
    have = {f[:-3] for f in os.listdir(os.path.join(ROOT, "h-edit_amd")) if f.startswith("main_") and f.endswith(".py")}
    assert have - {"main_edit_face_ef"} == set(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_default_namespace_is_the_parent_commits(name):
    got = vars(_driver(name).build_parser().parse_args([]))
    assert "native_text" not in got                     # opt-in: absent unless given
    assert got == GOLDEN[name]


@pytest.mark.parametrize("name", sorted(set(GOLDEN) - {"main_edit_face"}))
def test_native_text_is_still_accepted(name):
    assert _driver(name).build_parser().parse_args(["--native_text"]).native_text is True
