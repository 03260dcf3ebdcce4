"""Prediction on the GPU (moc_amd.predict, moc_meta_forward_models): every model's mixed scores are bit for bit those of
moc_meta_forward with that model alone, its pooled logits evaluation()'s; the ensemble agrees with a float64 oracle;
predict reproduces a training run's test metrics from its checkpoint; unlabeled bags from files work; and one predict
call runs phase A once whatever the number of models."""
import json
import os
from glob import glob

import numpy as np
import pandas as pd
import pytest
import torch

import helpers as H
from moc_amd import synth
from oracle import moc_oracle as O

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

# (C, storage, D, slide sizes, topj, topk, discard, R): N < topj, N not a multiple of 128, > 128-row tiles, a discard set
CASES = [
    (2, "fp32", 512, [1300, 7, 150, 2049, 64], 40, 10, (), 5),
    (3, "bf16", 512, [911, 129, 5, 1700], 30, 8, (), 2),
    (30, "fp16", 512, [640, 33, 1201, 250], 12, 6, (), 16),
    (30, "fp32", 512, [700, 260, 9], 10, 5, (), 2),
    (2, "bf16", 1024, [1500, 127, 3, 480], 25, 10, (), 16),
    (3, "fp32", 512, [1000, 300, 17, 530], 20, 7, ("delta_softmax",), 1),
    (2, "fp16", 1024, [2600, 90, 400], 400, 10, (), 5),
]


def _models(R, D, dev, seed):
    from moc_amd import main_moc as M
    out = []
    for r in range(R):
        torch.manual_seed(seed + 31 * r)
        m = M.senet(D, 4).to(dev)
        with torch.no_grad():                   # gates away from 0 / 1: every term of the mix matters
            m.model[2].weight.mul_(3.0)
        out.append(m)
    return out


def _setup(case, dev, seed=11):
    from moc_amd import main_moc as M
    C, st, D, sizes, j, K, discard, R = case
    W, We = synth.make_bank(seed, D, C)
    bags, labels = synth.make_slide_set(seed + 100, sizes, D, We, C)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    models = _models(R, D, dev, seed)
    args = H.make_args(C, j, K, discard)
    return W, We, bags, labels, models, args


@pytest.mark.parametrize("case", CASES, ids=[f"C{c[0]}-{c[1]}-D{c[2]}-R{c[7]}{'-discard' if c[6] else ''}" for c in CASES])
def test_each_model_bit_identical_and_ensemble_against_oracle(gpu_device, case):
    from moc_amd import engine, main_moc as M, predict as P
    dev = gpu_device
    C, st, D, sizes, j, K, discard, R = case
    W, We, bags, labels, models, args = _setup(case, dev)
    res = M.ResidentBags(bags, labels, dev, dtype=DT[st])
    bank = M._bank_for(res.X, dev)
    batch = res.eval_plan(bank.C, bank.Ce, j, K, list(discard))["batch"]
    batch.phase_a(bank, for_eval=True)
    use_bits = engine.eval_use_bits(discard)
    arena = engine.ModelArena([m.state_dict() for m in models], dev)
    mixed = torch.full((R, C, batch.total), float("nan"), dtype=torch.float32, device=dev)
    engine.meta_forward_models(batch, arena, R, mixed, 0, batch.n_slides, use_bits)
    got = mixed.cpu()
    n_sel = batch.n_sel.cpu().numpy()
    t, _ = batch.meta_ws()
    for r, model in enumerate(models):
        engine.meta_forward(batch, engine.MetaState(model), 0, batch.n_slides, use_bits, keep_hidden=False)
        ref = t["mixed"].cpu()
        for b in range(batch.n_slides):
            o, S = batch.row_off_host[b], int(n_sel[b])
            assert torch.equal(got[r, :, o:o + S], ref[:, o:o + S]), f"model {r} slide {b}: mixed differs"

    p = P.predict([m.state_dict() for m in models], res, dev, args)
    assert p.pooled.shape == (R, len(sizes), C) and p.labels.tolist() == labels
    for r, model in enumerate(models):
        pooled_eval, _, _ = M._eval_pass(res, dev, args, "eval", model=model)
        assert np.array_equal(p.pooled[r], pooled_eval.numpy()), f"model {r}: pooled differs from evaluation()"

    # float64 oracle on the stored (rounded) bags: mean over models of softmax(T * pooled)
    x64 = [b.to(DT[st]).double() for b in bags]
    probs = []
    for model in models:
        ref = O.Senet(D, 4).double()
        ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
        with torch.no_grad():                   # main_moc.py:481-495 per slide (O.evaluation's loop, without its AUC)
            pooled64 = []
            for x in x64:
                sr = O.slide_process(x, W.double(), We.double(), C, j, discard=discard)
                mixed64 = O.mix_eval(ref(sr["selected_feat"]), sr, discard)
                pooled64.append(O.pool_top(mixed64, [K])[1][K])
            pooled64 = torch.cat(pooled64, 0)
        probs.append(torch.softmax(pooled64 * M.CONCH_TEMPERATURE, dim=1).numpy())
    np.testing.assert_allclose(p.ensemble, np.mean(probs, axis=0), rtol=0, atol=1e-4)
    np.testing.assert_allclose(p.ensemble.sum(axis=1), 1.0, rtol=0, atol=1e-5)


def test_one_phase_a_for_all_models(gpu_device, monkeypatch):
    from moc_amd import engine, main_moc as M, predict as P
    dev = gpu_device
    W, We, bags, labels, models, args = _setup(CASES[1][:7] + (5,), dev)
    res = M.ResidentBags(bags, labels, dev, dtype=torch.bfloat16)
    calls = {"phase_a": 0, "scores": 0}
    orig_pa, orig_sc = engine.SlideBatch.phase_a, engine.SlideBatch.scores

    def phase_a(self, *a, **k):
        calls["phase_a"] += 1
        return orig_pa(self, *a, **k)

    def scores(self, *a, **k):
        calls["scores"] += 1
        return orig_sc(self, *a, **k)
    monkeypatch.setattr(engine.SlideBatch, "phase_a", phase_a)
    monkeypatch.setattr(engine.SlideBatch, "scores", scores)
    p = P.predict([m.state_dict() for m in models], res, dev, args)
    assert p.pooled.shape[0] == 5 and calls == {"phase_a": 1, "scores": 0}


def _run_dir(tmp_path):
    from moc_amd import run_moc
    rd = tmp_path / "train"
    res = run_moc.cli(["--synthetic", "24", "--shot", "4", "--epochs", "3", "--seed", "1", "--disable_tqdm",
                       "--result_dir", str(rd)])
    return rd, res


def test_predict_reproduces_the_training_runs_test_metrics(gpu_device, tmp_path):
    from moc_amd import predict as P
    rd, res = _run_dir(tmp_path)
    ckpt = glob(str(rd / "best_model_shot_4_fold_0.pt"))[0]
    best = json.load(open(rd / "best_results_shot_4_fold_0.json"))
    out = tmp_path / "pred"
    p, m = P.cli(["--ckpt", ckpt, "--synthetic", "24", "--shot", "4", "--fold", "0", "--split", "test", "--out", str(out),
                  "--disable_tqdm"])
    doc = json.load(open(out / "predictions.json"))
    assert doc["metrics"]["models"][0]["auc"] == best["test_at_best_val"]
    assert doc["metrics"]["models"][0]["acc"] == best["test_acc_at_best_val"]
    # R = 1: the ensemble is the model
    assert doc["metrics"]["ensemble"]["acc"] == best["test_acc_at_best_val"]
    df = pd.read_csv(out / "predictions.csv")
    assert len(df) == 24 and df["slide_id"].is_unique and "label" in df.columns


def test_unlabeled_slides_from_files(gpu_device, tmp_path):
    from moc_amd import datasets as DS, main_moc as M, predict as P
    dev = gpu_device
    C, D = 2, 512
    W, We = synth.make_bank(3, D, C)
    sizes = [700, 90, 1300, 260, 41]
    bags, labels = synth.make_slide_set(77, sizes, D, We, C)
    root = tmp_path / "root"
    wdir = root / "models" / "classifier_weights"
    wdir.mkdir(parents=True)
    torch.save(W, wdir / "weights_nsclc_conch.pt")
    torch.save(We, wdir / "weights_nsclc_ext_conch.pt")
    data = tmp_path / "bags"
    ids = [f"slide_{i}" for i in range(len(sizes))]
    rng = np.random.default_rng(0)
    for i, (sid, bag) in enumerate(zip(ids, bags)):
        if i % 2 == 0:
            DS.write_bag(str(data), sid, bag, coords=rng.integers(0, 50000, (sizes[i], 2)), fmt="pt")
        else:
            DS.write_bag(str(data), sid, bag, fmt="npy")
    pd.DataFrame({"slide_id": ids}).to_csv(tmp_path / "list.csv", index=False)
    pd.DataFrame({"slide_id": ids, "label": labels}).to_csv(tmp_path / "list_lab.csv", index=False)
    models = _models(2, D, dev, 5)
    ckpts = []
    for r, m in enumerate(models):
        ckpts.append(str(tmp_path / f"m{r}.pt"))
        torch.save(m.state_dict(), ckpts[-1])
    common = ["--ckpt"] + ckpts + ["--data_dir", str(data), "--root", str(root), "--topj", "30", "--topk", "8",
                                   "--disable_tqdm"]
    p, m = P.cli(common + ["--slides", str(tmp_path / "list.csv"), "--out", str(tmp_path / "u")])
    assert m is None and p.labels is None
    df = pd.read_csv(tmp_path / "u" / "predictions.csv", dtype={"slide_id": str})
    assert df["slide_id"].tolist() == ids and "label" not in df.columns
    names = ["LUAD", "LUSC"]
    ens = df[[f"prob_{n}" for n in names]].to_numpy(np.float64)
    np.testing.assert_allclose(ens.sum(axis=1), 1.0, atol=1e-5)
    per = np.stack([df[[f"m{r}_prob_{n}" for n in names]].to_numpy(np.float64) for r in range(2)])
    np.testing.assert_allclose(ens, per.mean(axis=0), rtol=0, atol=1e-7)
    assert df["pred"].tolist() == ens.argmax(axis=1).tolist()
    assert "metrics" not in json.load(open(tmp_path / "u" / "predictions.json"))
    # the labelled path over the same bags: the same numbers, plus metrics
    p2, m2 = P.cli(common + ["--slides", str(tmp_path / "list_lab.csv"), "--out", str(tmp_path / "l")])
    assert np.array_equal(p2.pooled, p.pooled) and np.array_equal(p2.ensemble, p.ensemble)
    assert p2.labels.tolist() == labels and len(m2["models"]) == 2
    # and a resident split of the same bags in memory
    args = H.make_args(C, 30, 8)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    res = M.ResidentBags(bags, labels, dev)
    p3 = P.predict([mm.state_dict() for mm in models], res, dev, args)
    assert np.array_equal(p3.pooled, p.pooled)
