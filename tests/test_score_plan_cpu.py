"""The score pass's launches are planned once, in moc_amd/csrc/moc_scores_plan.h: moc_scores and moc_scores_banks take form,
dynamic LDS, chunk and grid from score_plan.  tests/native/score_plan_host.cpp includes that header with g++ and, over a
grid of shapes, prints the plan and checks the streaming layout (StreamLds) against the kernels' hand-written carve.  The
plans must be the ones the two entries computed before the header existed (tests/golden/score_plan.json, written by
tests/golden/make_score_plan.py from those formulas), and the library's size queries must agree with the same recorder."""
import importlib.util
import itertools
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "score_plan.json")


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_score_plan", os.path.join(ROOT, "tests", "golden", "make_score_plan.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("score_plan") / "score_plan_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "moc_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "score_plan_host.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.splitlines(), r.stderr


def _flat(pt):
    return [x for v in pt for x in (v if isinstance(v, list) else [v])]


def test_the_streaming_layout_is_ordered_disjoint_aligned_and_holds_the_counter_word(printed):
    rc, lines, err = printed
    assert rc == 0 and lines[-1] == "bad=0", err


def test_plans_match_the_formulas_they_replaced(printed, gold):
    lines = printed[1]
    sections = [("scores", list(itertools.product(*gold["axes"].values())), gold["rows"]),
                ("banks", list(itertools.product(*gold["bank_axes"].values())), gold["bank_rows"]),
                ("extra", gold["extras"], gold["extra_rows"])]
    assert [len(p) for _, p, _ in sections] == [2700, 360, len(gold["extras"])]
    at, bad = 0, []
    for tag, points, rows in sections:
        assert len(points) == len(rows)
        for pt, want in zip(points, rows):
            head, kv = lines[at].split(" form=")[0].split(), dict(re.findall(r"(\w+)=(\d+)", lines[at]))
            at += 1
            assert head[0] == tag and list(map(int, head[1:])) == _flat(pt)
            got = [int(kv[f]) for f in gold["fields"]]
            if got != want:
                bad.append((tag, pt, dict(zip(gold["fields"], zip(got, want)))))
    assert lines[at].startswith("banks_max") and not bad, "%d grid points differ, first %s" % (len(bad), bad[:1])


def test_the_grid_does_not_pass_vacuously(gold):
    f = {n: i for i, n in enumerate(gold["fields"])}
    form, err = gold["forms"].index, gold["errs"].index
    rows = gold["rows"]
    seen = {(r[f["form"]], r[f["ticketed"]]) for r in rows if r[f["err"]] == 0}
    assert seen == {(form("stream"), 0), (form("stream"), 1), (form("wide_ring"), 0), (form("wide"), 0), (form("generic"), 0)}
    assert {r[f["err"]] for r in rows} == {err("ok"), err("slides_lds"), err("row_lds")}       # both "need(s) ... B of LDS" refusals
    points = list(itertools.product(*gold["axes"].values()))
    chunked = [(p, r) for p, r in zip(points, rows) if r[f["err"]] == 0 and r[f["form"]] == form("stream") and r[f["chunk"]] < p[3][0]]
    assert chunked and {r[f["NT"]] for _, r in chunked} >= {2, 3, 4}
    bank_points = list(itertools.product(*gold["bank_axes"].values()))
    assert any(r[f["err"]] == 0 and r[f["chunk"]] < p[3][0] and r[f["NT"]] == 1 for p, r in zip(bank_points, gold["bank_rows"]))
    assert {r[f["err"]] for r in gold["bank_rows"]} == {err("ok"), err("no_stream")}
    assert {r[f["unit"]] for r in rows if r[f["form"]] == form("stream") and r[f["err"]] == 0} == {8, 16}
    assert {r[f["gx"]] for r in rows if r[f["form"]] == form("stream") and r[f["err"]] == 0} >= {1, 256, 512}
    assert err("reserved") in {r[f["err"]] for r in gold["extra_rows"]}


def test_the_recorder_meets_its_hand_computed_anchors(recorder, gold):
    recorder.check_anchors()
    assert recorder.record() == gold


def test_the_printed_bank_table_is_the_one_the_gpu_suite_asserts(printed):
    table = [tuple(map(int, ln.split()[1:])) for ln in printed[1] if ln.startswith("banks_max")]
    assert table == [(256, 4, 3, 3), (512, 4, 3, 3), (1024, 2, 1, 1)]


def test_the_librarys_size_queries_agree_with_the_recorder(recorder, gold):
    """moc_bank_bytes, moc_bank_set_bytes and moc_scores_banks_max: pure host functions of the built library"""
    from moc_amd import _lib
    lib = _lib.lib()
    ax = gold["axes"]
    for D, dtype in itertools.product(ax["D"], ax["dtype"]):
        assert lib.moc_scores_banks_max(D, dtype) == recorder.banks_max(D, dtype), (D, dtype)
        for Ce in ax["Ce"]:
            assert lib.moc_bank_bytes(D, Ce, dtype) == recorder.bank_bytes(D, Ce, dtype), (D, Ce, dtype)
        for G in (1, 2, 3, 4):
            assert lib.moc_bank_set_bytes(D, G, dtype) == recorder.bank_set_bytes(D, G, dtype), (D, G, dtype)
    # the refusals of the three: sizes that are no batch, a dtype that is none
    assert lib.moc_bank_bytes(0, 3, 0) == lib.moc_bank_bytes(256, 0, 0) == lib.moc_bank_set_bytes(256, 0, 1) == 0
    assert lib.moc_scores_banks_max(300, 0) == lib.moc_scores_banks_max(256, 3) == lib.moc_scores_banks_max(0, 1) == 0
