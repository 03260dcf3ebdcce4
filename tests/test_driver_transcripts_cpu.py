"""The drivers' transcripts (tests/golden/driver_transcripts.json, written by tests/golden/make_driver_transcripts.py): with
the scripted stand-ins of tests/helpers_driver_fakes.py in place of moc_amd.main_moc's callables, `main`, `main_runs` and
`main_banks` print, call, write and return exactly what the record holds -- every line of stdout, every call and its
order, every file."""
import importlib.util
import json
import os

import pytest

import helpers as H

_spec = importlib.util.spec_from_file_location("make_driver_transcripts", os.path.join(H.GOLDEN_DIR, "make_driver_transcripts.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(REC.RECORD) as _f:
    GOLDEN = json.load(_f)
FIELDS = ("stdout", "calls", "files", "json", "checkpoints", "results")


def test_the_record_holds_the_recorder_s_scenarios():
    assert sorted(GOLDEN) == sorted(REC.SCENARIOS)
    assert all(sorted(GOLDEN[name]) == sorted(FIELDS) for name in GOLDEN)


@pytest.mark.parametrize("name", sorted(REC.SCENARIOS))
def test_scenario_matches_the_record(name):
    got = json.loads(json.dumps(REC.run_scenario(name)))
    for field in FIELDS:
        want = GOLDEN[name][field]
        if field == "stdout":                   # line by line: a failure names the first line that changed
            assert got[field].split("\n") == want.split("\n"), f"{name}: stdout"
        elif field == "calls":
            for i, (g, w) in enumerate(zip(got[field], want)):
                assert g == w, f"{name}: call {i}"
            assert len(got[field]) == len(want), f"{name}: number of calls"
        else:
            assert got[field] == want, f"{name}: {field}"


def test_the_scenarios_cover_what_they_are_there_for():
    """The record itself: a tie visits no test split, a run that stays at 0 writes no checkpoint and never sees the test
    split, and an epoch without an improvement makes no test call."""
    def test_calls(name):
        return [c for c in GOLDEN[name]["calls"] if any(s.endswith(":test") for s in c["splits"]) and c["fn"].startswith("evaluation")]
    assert len(test_calls("main")) == 2 and len(test_calls("main-no-zeroshot")) == 2
    assert GOLDEN["main"]["stdout"].count("Zero-shot Train") == 2 and "zs_results_shot_2_fold_3.json" in GOLDEN["main"]["files"]
    assert not any(f.startswith("zs_results") for f in GOLDEN["main-no-zeroshot"]["files"])
    assert GOLDEN["main-ablation"]["files"] == ["ablation_results_avg_shot_2_fold_3.json"]
    assert [c["fn"] for c in GOLDEN["main-ablation"]["calls"]] == ["ablation_evaluation"]
    for name, idle in (("runs-folds", "f1"), ("runs-shots-x-folds", "s1f1"), ("runs-hgrid", "c0f1"), ("runs-per-run-adam", "c0f1"),
                       ("banks", "A/f1")):
        rec = GOLDEN[name]
        assert list(rec["checkpoints"].values()).count(None) == 1
        assert not any(idle in c["models"] for c in test_calls(name))
        assert {m for c in test_calls(name) for m in c["models"]} == {m for c in rec["calls"] for m in c["models"]} - {idle}
    assert "[fold 2]" in GOLDEN["runs-folds"]["stdout"] and "[shot 2 fold 1]" in GOLDEN["runs-shots-x-folds"]["stdout"]
    assert "[topj 400 topk 10 topk+bottomk] [fold 0]" in GOLDEN["runs-hgrid"]["stdout"]
    assert "[seed 7 lr 0.0003 wd 0.0001] [fold 1]" in GOLDEN["runs-per-run-adam"]["stdout"]
    assert "[bank B] [fold 0]" in GOLDEN["banks"]["stdout"]
    # three epochs, improvements in the first and the last: evaluation_runs serves train + val every epoch and the test
    # splits twice (per configuration in a hyper-parameter grid)
    assert len([c for c in GOLDEN["runs-folds"]["calls"] if c["fn"] == "evaluation_runs"]) == 3 + 2
    assert len([c for c in GOLDEN["runs-hgrid"]["calls"] if c["fn"] == "evaluation_runs"]) == 2 * (3 + 2)
