"""Ensemble patch maps on the GPU (moc_meta_forward_dense_models, predict --patch_maps): the on-device reduction over R
models agrees with a float64 restatement of R single-model dense forwards, has zero spread for one model, leaves the
slots of other slides alone and is deterministic; end to end, the maps repeat predictions.csv and the single-model maps
bit for bit, from one phase A per chunk."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -7.25

# (C, storage, D, slide sizes, topj, topk, discard, R, sub): sub = leave the first and the last slide out of the launch
CASES = [
    (2, "fp32", 512, [1300, 7, 150, 2049, 64], 40, 10, (), 3, True),
    (3, "bf16", 512, [911, 129, 5, 1700], 30, 8, (), 16, False),
    (30, "fp16", 512, [640, 33, 1201, 250], 12, 6, (), 3, True),
    (30, "fp32", 512, [700, 260, 9], 10, 5, (), 16, False),
    (2, "bf16", 1024, [1500, 127, 3, 480], 25, 10, (), 1, True),
    (3, "fp32", 512, [1000, 300, 17, 530], 20, 7, ("delta_softmax",), 3, False),
    (2, "fp16", 1024, [2600, 90, 400], 400, 10, (), 16, True),
    (3, "fp32", 1024, [513, 2000, 40], 20, 5, (), 1, False),
]


def _models(R, D, dev, seed):
    from moc_amd import main_moc as M
    out = []
    for r in range(R):
        torch.manual_seed(seed + 31 * r)
        m = M.senet(D, 4).to(dev)
        with torch.no_grad():                   # gates away from 0 / 1, models that disagree
            m.model[2].weight.mul_(3.0)
        out.append(m)
    return out


def _batch(case, dev, seed=11):
    from moc_amd import main_moc as M
    C, st, D, sizes, j, K, discard, R, sub = case
    W, We = synth.make_bank(seed, D, C)
    bags, labels = synth.make_slide_set(seed + 100, sizes, D, We, C)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    res = M.ResidentBags(bags, labels, dev, dtype=DT[st])
    bank = M._bank_for(res.X, dev)
    batch = res.eval_plan(bank.C, bank.Ce, j, K, list(discard))["batch"]
    batch.phase_a(bank, for_eval=True)
    return batch, _models(R, D, dev, seed)


def _run(batch, arena, R, scale, slide0, n, use_bits):
    dev = batch.device
    pm = torch.full((batch.C, batch.total), SENTINEL, dtype=torch.float32, device=dev)
    ps = torch.full((batch.C, batch.total), SENTINEL, dtype=torch.float32, device=dev)
    gm = torch.full((batch.total, 4), SENTINEL, dtype=torch.float32, device=dev)
    from moc_amd import engine
    engine.meta_forward_dense_models(batch, arena, R, scale, pm, ps, gm, slide0, n, use_bits)
    torch.cuda.synchronize()
    return pm.cpu(), ps.cpu(), gm.cpu()


@pytest.mark.parametrize("case", CASES, ids=[f"C{c[0]}-{c[1]}-D{c[2]}-R{c[7]}{'-discard' if c[6] else ''}{'-sub' if c[8] else ''}"
                                             for c in CASES])
def test_against_single_model_dense_launches(gpu_device, case):
    from moc_amd import engine, main_moc as M
    dev = gpu_device
    C, st, D, sizes, j, K, discard, R, sub = case
    batch, models = _batch(case, dev)
    ns = batch.n_slides
    slide0, n = (1, ns - 2) if sub else (0, ns)
    use_bits = engine.eval_use_bits(discard)
    scale = M.CONCH_TEMPERATURE
    arena = engine.ModelArena([m.state_dict() for m in models], dev)
    pm, ps, gm = _run(batch, arena, R, scale, slide0, n, use_bits)

    # R single-model dense forwards, restated in float64
    mixed, gates = [], []
    for model in models:
        mx = torch.empty((C, batch.total), dtype=torch.float32, device=dev)
        g = torch.empty((batch.total, 4), dtype=torch.float32, device=dev)
        engine.meta_forward_dense(batch, engine.MetaState(model), slide0, n, use_bits, g, mx)
        mixed.append(mx.cpu().double())
        gates.append(g.cpu().double())
    torch.cuda.synchronize()
    lo, hi = batch.row_off_host[slide0], batch.row_off_host[slide0 + n]
    mixed = torch.stack(mixed)[:, :, lo:hi]
    p = torch.softmax(float(np.float32(scale)) * mixed, dim=1)          # [R, C, rows]
    mean = p.mean(dim=0)
    std = ((p - mean) ** 2).mean(dim=0).sqrt()
    gmean = torch.stack(gates)[:, lo:hi].mean(dim=0)
    np.testing.assert_allclose(pm[:, lo:hi].double().numpy(), mean.numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(ps[:, lo:hi].double().numpy(), std.numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(gm[lo:hi].double().numpy(), gmean.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(pm[:, lo:hi].double().sum(dim=0).numpy(), 1.0, rtol=0, atol=1e-5)
    if R == 1:
        assert torch.all(ps[:, lo:hi] == 0), "one model: the std is exactly 0"
        assert torch.equal(gm[lo:hi], gates[0][lo:hi].float()), "one model: the mean gates are the model's"
    # slots of the slides outside the launch keep the sentinel
    for t in (pm, ps):
        assert torch.all(t[:, :lo] == SENTINEL) and torch.all(t[:, hi:] == SENTINEL)
    assert torch.all(gm[:lo] == SENTINEL) and torch.all(gm[hi:] == SENTINEL)
    # deterministic: a second call gives the same bits
    pm2, ps2, gm2 = _run(batch, arena, R, scale, slide0, n, use_bits)
    assert torch.equal(pm, pm2) and torch.equal(ps, ps2) and torch.equal(gm, gm2)


def test_optional_outputs(gpu_device):
    """prob_std and gates_mean may be NULL; prob_mean is the same bits either way."""
    from moc_amd import engine, main_moc as M
    dev = gpu_device
    case = CASES[0]
    batch, models = _batch(case, dev)
    arena = engine.ModelArena([m.state_dict() for m in models], dev)
    pm, _, _ = _run(batch, arena, len(models), M.CONCH_TEMPERATURE, 0, batch.n_slides, 15)
    alone = torch.full((batch.C, batch.total), SENTINEL, dtype=torch.float32, device=dev)
    engine.meta_forward_dense_models(batch, arena, len(models), M.CONCH_TEMPERATURE, alone, None, None, 0, batch.n_slides, 15)
    assert torch.equal(alone.cpu(), pm)


def test_predict_patch_maps_end_to_end(gpu_device, tmp_path, monkeypatch):
    from moc_amd import engine, main_moc as M, patch_maps as PM, predict as P, run_moc
    dev = gpu_device
    models = _models(3, 512, dev, 21)
    ckpts = []
    for r, m in enumerate(models):
        ckpts.append(str(tmp_path / f"f{r}.pt"))
        torch.save(m.state_dict(), ckpts[-1])
    calls = {"phase_a": 0, "chunks": 0}
    orig_pa, orig_eb = engine.SlideBatch.phase_a, M._eval_batches

    def phase_a(self, *a, **k):
        calls["phase_a"] += 1
        return orig_pa(self, *a, **k)

    def eval_batches(*a, **k):
        bank, batches = orig_eb(*a, **k)

        def counted():
            for item in batches:
                calls["chunks"] += 1
                yield item
        return bank, counted()
    monkeypatch.setattr(engine.SlideBatch, "phase_a", phase_a)
    monkeypatch.setattr(M, "_eval_batches", eval_batches)
    out = tmp_path / "pred"
    p, m = P.cli(["--ckpt"] + ckpts + ["--synthetic", "12", "--shot", "4", "--fold", "0", "--split", "test",
                                       "--out", str(out), "--disable_tqdm", "--patch_maps"])
    assert calls["chunks"] >= 1 and calls["phase_a"] == calls["chunks"]
    monkeypatch.undo()

    df = pd.read_csv(out / "predictions.csv", dtype={"slide_id": str})
    index = json.load(open(out / "patch_maps" / "index.json"))
    assert sorted(index) == sorted(df["slide_id"].tolist()) and len(index) == 12
    names = p.classes
    emaps = {}
    for i, sid in enumerate(df["slide_id"]):
        em = PM.load_ensemble_map(str(out / "patch_maps" / index[sid]["file"]))
        emaps[sid] = em
        row = df.iloc[i]
        assert np.array_equal(em.probabilities, np.array([row[f"prob_{c}"] for c in names], dtype=np.float32)), sid
        assert em.pred == int(row["pred"]) == index[sid]["pred"] and em.label == int(row["label"])
        assert np.array_equal(em.pooled, p.pooled[:, i])
        N = em.coords.shape[0]
        assert em.prob_mean.shape == em.prob_std.shape == (N, len(names)) and em.gates_mean.shape == (N, 4)
        assert em.evidence.shape[:2] == (3, len(names))

    # the single-model maps of the same split
    ra = run_moc.get_args([])
    for k, v in dict(synthetic=12, shot=4, fold=0, disable_tqdm=True).items():
        setattr(ra, k, v)
    loader = run_moc.prepare(ra, dev)[2]
    args = H.make_args(ra.n_classes, 10, 10)
    for r, model in enumerate(models):
        maps = PM.patch_maps(model, loader, dev, args)
        assert len(maps) == len(emaps)
        for pm in maps:
            em = emaps[PM.slide_id_of(pm.path)]
            assert np.array_equal(em.evidence[r], pm.evidence), f"model {r}: evidence differs"
            if r == 0:
                assert np.array_equal(em.logits, pm.logits) and np.array_equal(em.selected, pm.selected)
                assert np.array_equal(em.zs_evidence, pm.zs_evidence) and np.array_equal(em.coords, pm.coords)
