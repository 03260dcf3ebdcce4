"""The evaluation family against the record of the commit before its loops were shared (tests/golden/eval_family.json,
written by tests/golden/make_eval_family.py): every public form, in every situation, returns the identical result (floats
by float.hex(), arrays by SHA-256), leaves the identical `repeat_num`, and calls the identical sequence of library
entries.  The other GPU tests compare one form with another; they cannot see a mistake in what the forms share."""
import pytest
import torch

import helpers_eval_family as F
from moc_amd import engine
from moc_amd import main_moc as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(F.SPLITS))
def test_every_form_is_the_record(gpu_device, name, monkeypatch):
    record = F.load_record()[name]
    S = F.split(name, gpu_device)
    log = F.EntryLog(engine.lib)
    monkeypatch.setattr(engine, "lib", log)
    monkeypatch.setattr(M, "zeroshot_weights", S.banks[0][0])
    monkeypatch.setattr(M, "zeroshot_weights_ext", S.banks[0][1])
    monkeypatch.setattr(M.evaluation_runs, "last_pooled", None, raising=False)
    cells = F.cells(S)
    assert [c[0] for c in cells] == list(record), "the record holds other calls than the test makes"
    with torch.random.fork_rng(devices=[]):
        for cid, sit, datasets, thunk in cells:
            got = F.run_cell(S, log, sit, datasets, thunk, F.setattr_undo)
            want = record[cid]
            assert got["result"] == want["result"], (cid, "result")
            assert got["repeat_num"] == want["repeat_num"], (cid, "repeat_num", got["repeat_num"], want["repeat_num"])
            assert got["entries"] == want["entries"], (cid, "entries", got["entries"], want["entries"])
