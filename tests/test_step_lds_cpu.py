"""The step kernels' dynamic LDS is described once, in moc_amd/csrc/moc_step_lds.h: the kernels carve with the layouts the
host sizes the launches with.  tests/native/step_lds_host.cpp includes that header with g++ and, over a grid of shapes,
prints what every launch asks for and checks each layout's order, extents, alignment and pad.  The totals must be the
ones the host formulas gave before the layouts existed (tests/golden/step_lds.json, written by
tests/golden/make_step_lds.py from those formulas): the bytes of a launch decide how many workgroups share a CU."""
import itertools
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_lds.json")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("step_lds") / "step_lds_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "moc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "step_lds_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.splitlines(), r.stderr


def test_every_layout_is_ordered_disjoint_aligned_and_padded_to_its_total(printed):
    rc, lines, err = printed
    tail = dict(re.findall(r"(\w+)=(\d+)", lines[-1]))
    assert rc == 0 and tail["bad"] == "0", err
    # pool_step_kernel's launch is now checked against its limit: never for a shape step_plan's pool_one admits
    assert tail["pool_one_over"] == "0"


def test_limits_did_not_move(printed):
    limits = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", printed[1][0])}
    lds = 160 * 1024 - 64
    assert limits == {"finish": 159 * 1024, "pool_step": 160 * 1024, "narrow": lds, "tiles": lds, "wide": lds}


def test_totals_match_the_formulas_they_replaced(printed):
    gold = json.load(open(GOLDEN))
    points = list(itertools.product(*gold["axes"].values()))
    rows = printed[1][1:-1]
    assert list(gold["axes"]) == ["C", "K", "D", "esz", "train"] and len(points) == len(rows) == len(gold["rows"]) == 2016
    bad = []
    for pt, line, want in zip(points, rows, gold["rows"]):
        head, kv = line.split(" finish=")[0], dict(re.findall(r"(\w+)=(\d+)", line))
        assert tuple(map(int, head.split())) == pt
        got = [int(kv[f]) for f in gold["fields"]]
        if got != want:
            bad.append((pt, dict(zip(gold["fields"], zip(got, want)))))
    assert not bad, "%d grid points differ, first %s" % (len(bad), bad[0])
    # the grid does not pass vacuously: chunked and unchunked wide shapes, both list caps, shapes over the limit
    col = {f: [r[i] for r in gold["rows"]] for i, f in enumerate(gold["fields"])}
    pairs = [c * k for c, k, *_ in points]
    assert any(p > pch for p, pch in zip(pairs, col["pch"])) and any(p <= pch for p, pch in zip(pairs, col["pch"]))
    assert len(set(col["wide_cap"])) > 1 and min(col["narrow"]) < lds_max() < max(col["narrow"])


def lds_max():
    return 160 * 1024 - 64


def test_the_recorder_meets_its_hand_computed_anchors():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_step_lds", os.path.join(ROOT, "tests", "golden", "make_step_lds.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.check_anchors()
    assert m.record() == json.load(open(GOLDEN))
