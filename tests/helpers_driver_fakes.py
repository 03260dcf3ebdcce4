"""Scripted stand-ins for what the drivers of moc_amd.run_moc call in moc_amd.main_moc (test-side only), shared by
tests/golden/make_driver_transcripts.py (which writes tests/golden/driver_transcripts.json) and
tests/test_driver_transcripts_cpu.py (which compares with it).  With them `main`, `main_runs` and `main_banks` run on the
CPU: they print, write their JSONs and save their checkpoints as ever; only the numbers come from a table.

A model is a two-parameter module that carries its run id and counts its training passes; a split carries (run, kind).
A stand-in appends one line to the call log -- its name, the run ids of its models, `run:kind` of its splits (and the banks
it was given), topj / topk / discard_classifiers of its `args` and its sorted keyword names -- and returns metrics that
depend on (run, split kind, epoch) alone: the validation AUC from the scenario's table, everything else from fixed
integer arithmetic."""
from __future__ import annotations

import contextlib

import torch

from moc_amd import main_moc as M

KINDS = ("train", "val", "test")
NAMES = ("train_runs", "evaluation_runs", "evaluation_banks", "zs_evaluation", "zs_evaluation_banks", "pack_splits", "train",
         "evaluation", "ablation_evaluation")


class Model(torch.nn.Module):
    def __init__(self, run):
        super().__init__()
        self.run, self.passes = run, 0
        self.scale = torch.nn.Parameter(torch.ones(2))
        self.shift = torch.nn.Parameter(torch.zeros(1))


class Split:
    def __init__(self, run, kind):
        self.run, self.kind = run, kind

    def __repr__(self):
        return f"{self.run}:{self.kind}"


def splits(run):
    return tuple(Split(run, kind) for kind in KINDS)


class Fakes:
    """`val_auc[run]` = the validation AUC of that run's model after epoch 0, 1, ...; the position of a run in the dict is
    what tells its other numbers from its neighbours'."""

    def __init__(self, val_auc):
        self.val_auc = {run: list(v) for run, v in val_auc.items()}
        self.order = {run: i for i, run in enumerate(val_auc)}
        self.calls = []

    # -------------------------------------------------------------- the table
    def metrics(self, run, kind, epoch):
        o, k = self.order.get(run, len(self.order)), KINDS.index(kind)
        if epoch is None:                           # a zero-shot or ablation pass: no model
            return {"loss": (900 + 7 * o + k) / 1000, "acc": (300 + 11 * o + 3 * k) / 1000, "auc": (400 + 13 * o + 5 * k) / 1000}
        auc = self.val_auc[run][epoch] if kind == "val" else (500 + 100 * k + 13 * o + 3 * epoch) / 1000
        return {"loss": (800 - 50 * epoch + 7 * o + k) / 1000, "acc": (450 + 50 * k + 11 * o + 2 * epoch) / 1000, "auc": auc}

    def log(self, name, models=(), loaders=(), args=None, banks=None, kw=()):
        def cfg(a):
            return None if a is None else [a.topj, a.topk, list(a.discard_classifiers or ())]
        line = {"fn": name, "models": [m.run for m in models], "splits": [repr(ld) for ld in loaders],
                "args": [cfg(a) for a in args] if isinstance(args, list) else cfg(args), "kw": sorted(kw)}
        if banks is not None:
            line["banks"] = list(banks)
        self.calls.append(line)

    # -------------------------------------------------------------- the stand-ins (signatures of moc_amd.main_moc)
    def train(self, model, train_loader, optimizer, device, args):
        self.log("train", [model], [train_loader], args)
        model.passes += 1

    def train_runs(self, models, train_loaders, optimizers, device, args, **kw):
        assert len(models) == len(train_loaders) == len(optimizers)
        self.log("train_runs", models, train_loaders, args, banks=kw.get("banks"), kw=kw)
        for m in models:
            m.passes += 1

    def evaluation(self, model, loader, device, args):
        self.log("evaluation", [model], [loader], args)
        return self.metrics(model.run, loader.kind, model.passes - 1)

    def evaluation_runs(self, models, loaders, device, args):
        assert len(models) == len(loaders)
        self.log("evaluation_runs", models, loaders, args)
        return [self.metrics(m.run, ld.kind, m.passes - 1) for m, ld in zip(models, loaders)]

    def evaluation_banks(self, models, loader, device, args, banks):
        assert len(models) == len(banks)
        self.log("evaluation_banks", models, [loader], args, banks=banks)
        return [self.metrics(m.run, loader.kind, m.passes - 1) for m in models]

    def zs_evaluation(self, loader, device, args):
        self.log("zs_evaluation", (), [loader], args)
        return self.metrics(loader.run, loader.kind, None)

    def zs_evaluation_banks(self, loader, device, args, banks):
        self.log("zs_evaluation_banks", (), [loader], args, banks=banks)
        return [self.metrics(f"{b}/{loader.run}", loader.kind, None) for b in banks]

    def ablation_evaluation(self, loader, device, args):
        self.log("ablation_evaluation", (), [loader], args)
        return self.metrics(loader.run, loader.kind, None)

    def pack_splits(self, loaders):
        self.log("pack_splits", (), loaders, None)


@contextlib.contextmanager
def installed(fakes):
    """moc_amd.main_moc's nine callables replaced by `fakes`' for the length of the block."""
    kept = {name: getattr(M, name) for name in NAMES}
    try:
        for name in NAMES:
            setattr(M, name, getattr(fakes, name))
        yield fakes
    finally:
        for name, fn in kept.items():
            setattr(M, name, fn)
