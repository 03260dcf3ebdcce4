#!/usr/bin/env python3
"""Write tests/golden/eval_family.json: what every public form of the evaluation family (moc_amd.main_moc evaluation,
zs_evaluation, ablation_evaluation, the sweeps, the bank forms, evaluation_runs; predict.predict; patch_maps.patch_maps)
returns on three small generated splits, what it leaves in `repeat_num`, and which library entries it calls in which
order -- per situation (repeat_num None / real_len + 3 / 4, a plain loader, at least three chunks).

Run on the GPU, on the commit whose behaviour is to be kept:

    python -B tests/golden/make_eval_family.py

The inputs come from moc_amd.synth with fixed seeds (tests/helpers_eval_family.py); tests/test_gpu_eval_family.py rebuilds
them and compares with `==`.  Every form is called twice; a cell whose two outcomes differ is not written (and the run
fails), since such a cell could not be compared exactly."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch

import helpers_eval_family as F
from moc_amd import engine
from moc_amd import main_moc as M


def main(out_path=F.RECORD):
    dev = torch.device("cuda:0")
    log = F.EntryLog(engine.lib)
    engine.lib = log
    record, refused = {}, []
    for name in F.SPLITS:
        S = F.split(name, dev)
        M.set_classifier_bank(*S.banks[0])
        record[name] = {}
        for cid, sit, datasets, thunk in F.cells(S):
            first = F.run_cell(S, log, sit, datasets, thunk, F.setattr_undo)
            again = F.run_cell(S, log, sit, datasets, thunk, F.setattr_undo)
            if first != again:
                refused.append(f"{name}::{cid}")
                print(f"{name}::{cid} differs in {[k for k in first if first[k] != again[k]]}: "
                      f"{first['entries']} / {again['entries']}", flush=True)
                continue
            record[name][cid] = again
        print(f"{name}: {len(record[name])} cells", flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    F.save_record(record, out_path)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes")
    if refused:
        raise SystemExit(f"two calls differed, not written: {refused}")


if __name__ == "__main__":
    main(*sys.argv[1:])
