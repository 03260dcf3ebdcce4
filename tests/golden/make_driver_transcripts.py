#!/usr/bin/env python3
"""Write tests/golden/driver_transcripts.json: what `main`, `main_runs` and `main_banks` of moc_amd.run_moc print, call,
write and return when the callables of moc_amd.main_moc are the scripted stand-ins of tests/helpers_driver_fakes.py.

Run on the CPU, on the commit whose behaviour is to be kept:

    python -B tests/golden/make_driver_transcripts.py

Per scenario: stdout (the temporary directory spelled <TMP>), the call log, the sorted file tree, every JSON file's text,
per run the `state_dict` keys of its checkpoint (null: none was written) and the returned results.
tests/test_driver_transcripts_cpu.py runs `record()` again and compares field by field."""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch

import helpers_driver_fakes as F
from moc_amd import run_moc

RECORD = os.path.join(HERE, "driver_transcripts.json")
TOKEN = "<TMP>"
DEVICE = torch.device("cpu")
# four runs, three epochs: improve / tie / improve; never above 0 (no checkpoint, no test pass); improve / fall / improve;
# improve / tie / fall.  Nobody improves in epoch 1: that epoch makes no test call at all.
FOUR = ([0.6, 0.6, 0.7], [0.0, 0.0, 0.0], [0.5, 0.4, 0.8], [0.3, 0.3, 0.2])
ONE = [0.5, 0.5, 0.4, 0.9]          # improve, tie (no test pass), fall, improve


def _args(tmp, *flags):
    return run_moc.get_args(["--result_dir", tmp, "--disable_tqdm", *flags])


def _adam(models):
    return [torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4) for m in models]


def _main(tmp, zeroshot=True, ablation="none"):
    a = _args(tmp, "--epochs", "4", "--shot", "2", "--fold", "3", "--ablation_study", ablation)
    a.check_zeroshot = zeroshot
    fakes = F.Fakes({"r0": ONE})
    model = F.Model("r0")
    with F.installed(fakes):
        res = run_moc.main(a, model, _adam([model])[0], *F.splits("r0"), DEVICE)
    return fakes, [res]


def _main_runs(tmp, ids, args_list, **kw):
    fakes = F.Fakes(dict(zip(ids, FOUR)))
    models = [F.Model(i) for i in ids]
    with F.installed(fakes):
        res = run_moc.main_runs(args_list, models, _adam(models), [F.splits(i) for i in ids], DEVICE,
                                generators=[torch.Generator() for _ in ids], **kw)
    return fakes, res


def _folds(tmp):
    base = _args(tmp, "--epochs", "3", "--shot", "4", "--folds", "0,1,2,3")
    args_list = []
    for fold in range(4):
        a = copy.copy(base)
        a.fold = fold
        args_list.append(a)
    return _main_runs(tmp, [f"f{f}" for f in range(4)], args_list)


def _shots(tmp):
    base = _args(tmp, "--epochs", "3", "--shots", "1,2", "--folds", "0,1")
    args_list = []
    for shot, fold in run_moc.pairs_of_rank(base.shots, base.folds, base.shot, base.fold, 0, 1):
        a = copy.copy(base)
        a.shot, a.fold, a.result_dir = shot, fold, run_moc.run_result_dir(base, shot)
        args_list.append(a)
    return _main_runs(tmp, [f"s{a.shot}f{a.fold}" for a in args_list], args_list)


def _hgrid(tmp):
    base = _args(tmp, "--epochs", "3", "--shot", "4", "--topjs", "100,400", "--discard_sets", "topk+bottomk", "--folds", "0,1")
    args_list = run_moc.hgrid_runs(base, run_moc.hgrid_configs(base), [0, 1])
    return _main_runs(tmp, [f"c{r // 2}f{a.fold}" for r, a in enumerate(args_list)], args_list)


def _optgrid(tmp):
    base = _args(tmp, "--epochs", "3", "--shot", "4", "--seeds", "7", "--lrs", "3e-4,1e-3", "--folds", "0,1")
    args_list = run_moc.optgrid_runs(base, run_moc.optgrid_cells(base), [0, 1])
    return _main_runs(tmp, [f"c{r // 2}f{a.fold}" for r, a in enumerate(args_list)], args_list, per_run_adam=True)


def _banks(tmp):
    base = _args(tmp, "--epochs", "3", "--shot", "4", "--seed", "1", "--folds", "0,1")
    names, folds = ["A", "B"], [0, 1]
    args_list = run_moc.bankgrid_runs(base, names, folds)
    ids = [f"{a.bank}/f{a.fold}" for a in args_list]
    fakes = F.Fakes(dict(zip(ids, FOUR)))
    models = [F.Model(i) for i in ids]
    with F.installed(fakes):
        res = run_moc.main_banks(args_list, names, folds, models, _adam(models), [F.splits(f"f{f}") for f in folds], DEVICE,
                                 [torch.Generator() for _ in ids], names)
    return fakes, res


SCENARIOS = {
    "main": _main,
    "main-no-zeroshot": lambda tmp: _main(tmp, zeroshot=False),
    "main-ablation": lambda tmp: _main(tmp, ablation="avg"),
    "runs-folds": _folds,
    "runs-shots-x-folds": _shots,
    "runs-hgrid": _hgrid,
    "runs-per-run-adam": _optgrid,
    "banks": _banks,
}


def run_scenario(name):
    """-> the scenario's record (JSON-ready)."""
    with tempfile.TemporaryDirectory() as tmp:
        def tok(text):
            return text.replace(tmp, TOKEN)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            fakes, results = SCENARIOS[name](tmp)
        files = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)
        texts = {}
        for rel in files:
            if rel.endswith(".json"):
                with open(os.path.join(tmp, rel)) as f:
                    texts[rel] = tok(f.read())
        checkpoints = {}
        for r in results:
            path = r.get("best_model_path")
            if path is not None:
                checkpoints[os.path.relpath(path, tmp)] = sorted(torch.load(path, map_location="cpu")) if os.path.exists(path) else None
        return {"stdout": tok(out.getvalue()), "calls": fakes.calls, "files": files, "json": texts, "checkpoints": checkpoints,
                "results": json.loads(tok(json.dumps(results)))}


def record():
    return {name: run_scenario(name) for name in SCENARIOS}


def main(out_path=RECORD):
    rec = record()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out_path}: {len(rec)} scenarios, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
