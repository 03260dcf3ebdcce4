"""The ring form of the score pass in the launch plan (moc_amd/csrc/moc_scores_plan.h, MOC_SCORES_RING): when score_plan
chooses it, what it refuses, how many ring slots a launch gets -- restated here from the two LDS figures it is derived
from -- and the MOC_SCORE_RING switch of moc_amd.engine.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOC_F32 = 0


def fks_lds_bytes(D, H=64):
    """moc_meta_forward.hip: the training forward's dynamic LDS (a static_assert there ties SCORE_RING_BESIDE_LDS to it)"""
    return 3 * 16 * D * 2 + 4 * 16 * (H + 4) * 4 + 16 * (H + 4) * 4 + 16 * 4 * 4 + 4 * (H + 4) * 4


def ring_bytes(D, n, slots):
    meta_end = (D // 16) * 1024 + slots * 16384 + 3 * 16 * 17 * 4 + 24 * n + 4
    return (meta_end + 15) // 16 * 16 + 24 * slots


def ring_slots(D, n):
    """the most 16 KiB slots whose launch leaves the forward's LDS free on a 160 KiB CU; the form needs three, takes eight"""
    s = 0
    while s < 8 and ring_bytes(D, n, s + 1) + fks_lds_bytes(512) <= 160 * 1024:
        s += 1
    return s if s >= 3 else 0


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("score_ring_plan") / "score_ring_plan_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "moc_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "score_ring_plan_host.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "bad=0", r.stderr
    lines = r.stdout.splitlines()
    const = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[0])}
    rows = []
    for ln in lines[1:-1]:
        head, p0, p1 = ln.split(" | ")
        rows.append((list(map(int, head.split()[1:])), {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p0)},
                     {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p1)}))
    return const, rows


def test_the_constants_are_the_two_lds_figures(printed):
    const, _ = printed
    assert const["max_lds"] == 160 * 1024 and const["beside"] == fks_lds_bytes(512) == 72256 and const["slot"] == 16 * 1024
    assert (const["min"], const["max"], const["form_ring"]) == (3, 8, 4)
    header = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"MOC_SCORES_RING = 64\b", header)
    from moc_amd import _lib
    assert _lib.MOC_SCORES_RING == 64 and _lib.SCORE_FORM_RING == const["form_ring"]


def test_the_plans_choice_for_every_flag_and_shape(printed):
    const, rows = printed
    assert len(rows) == 4 * 3 * 5 * 5 * 4
    seen = set()
    for (D, dt, Ce, n, total, ticket, reserved), p0, p1 in rows:
        assert p0["form"] != const["form_ring"], "never without the bit"
        if ticket or reserved:
            assert p1["err"] == const["err_ring_ticket"], "the bit beside a ticket or a reserved set is refused, whatever the shape"
            seen.add("refused")
            continue
        slots = ring_slots(D, n) if (dt == MOC_F32 and Ce <= 16) else 0
        if slots:
            assert (p1["form"], p1["err"], p1["unit"], p1["chunk"]) == (const["form_ring"], 0, slots, n)
            assert p1["smem"] == ring_bytes(D, n, slots) and p1["smem"] + fks_lds_bytes(512) <= 160 * 1024
            assert p1["gx"] == min(256, (total + 15) // 16 + 2 * n)
            seen.add(("ring", D, slots))
        else:
            assert all(p1[k] == p0[k] for k in ("form", "unit", "smem", "gx", "err")), "other shapes keep their plan"
            seen.add(("kept", dt == MOC_F32, Ce <= 16))
    # the benchmark's shape has three slots, D = 256 four; 16-bit bags, wider banks and D = 1024 keep their kernels
    assert {("ring", 512, 3), ("ring", 256, 4), ("kept", False, True), ("kept", True, False), ("kept", True, True), "refused"} <= seen
    assert ring_slots(512, 32) == 3 and ring_slots(256, 32) == 4 and ring_slots(1024, 32) == 0 and ring_slots(768, 32) == 0


def test_the_step_kernels_launch_limit_is_no_budget():
    """lds::TILE_MAX_LDS is the limit the step kernels are raised to -- the whole CU less 64 bytes -- so nothing fits beside
    it by construction; the ring is sized against the forward's LDS alone (moc_scores_plan.h says so)."""
    src = open(os.path.join(ROOT, "moc_amd", "csrc", "moc_step_lds.h")).read()
    assert re.search(r"FS_MAX_DYN_LDS = 160 \* 1024 - 64;", src) and re.search(r"TILE_MAX_LDS = FS_MAX_DYN_LDS", src)
    assert ring_bytes(256, 1, 3) + 160 * 1024 - 64 > 160 * 1024


def test_the_switch_parses_three_values():
    from moc_amd import engine
    assert [engine.score_ring_mode(v) for v in (None, "", "0", "lookahead", " ALL ")] == ["0", "0", "0", "lookahead", "all"]
    for v in ("1", "on", "look"):
        with pytest.raises(ValueError, match="MOC_SCORE_RING"):
            engine.score_ring_mode(v)
    assert engine.SCORE_RING == engine.score_ring_mode(os.environ.get("MOC_SCORE_RING", "lookahead"))
