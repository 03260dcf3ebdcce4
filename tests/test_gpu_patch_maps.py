"""Patch maps on the GPU (moc_amd.patch_maps, moc_meta_forward_dense): the dense forward gives every union row the bits the
prediction's own forward gives it, `pooled` is the evaluation's logits, `evidence` is what pooling averaged, and every
field agrees with the float64 oracle on the stored bags; coordinates survive ingestion; the driver writes the maps and
reproduces them from a saved checkpoint."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import helpers as H
from moc_amd import synth
from oracle import moc_oracle as O

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

# (C, storage, D, slide sizes, topj, topk, discard): sizes cover N < topj, N < K, N not a multiple of 128, > 128-row tiles
CASES = [
    (2, "fp32", 512, [1300, 7, 150, 2049, 64], 40, 10, ()),
    (3, "bf16", 512, [911, 129, 5, 1700], 30, 8, ()),
    (30, "fp16", 512, [640, 33, 1201, 250], 12, 6, ()),
    (30, "fp32", 512, [700, 260, 9], 10, 5, ()),
    (2, "bf16", 1024, [1500, 127, 3, 480], 25, 10, ()),
    (3, "fp32", 512, [1000, 300, 17, 530], 20, 7, ("delta_softmax",)),
]


def _setup(case, dev, seed=11):
    from moc_amd import main_moc as M
    C, st, D, sizes, j, K, discard = case
    W, We = synth.make_bank(seed, D, C)
    bags, labels = synth.make_slide_set(seed + 100, sizes, D, We, C)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    torch.manual_seed(seed)
    model = M.senet(D, 4).to(dev)
    with torch.no_grad():                       # gates away from 0 / 1: every term of the mix matters
        model.model[2].weight.mul_(3.0)
    args = H.make_args(C, j, K, discard)
    return C, st, D, sizes, j, K, discard, W, We, bags, labels, model, args


def _oracle_rows(x64, W64, We64, model, C, discard):
    """float64 over ALL rows of one stored bag: logits, gates, the eval mix."""
    lin1, lin2 = model.model[0], model.model[2]
    W1, b1 = lin1.weight.detach().cpu().double(), lin1.bias.detach().cpu().double()
    W2, b2 = lin2.weight.detach().cpu().double(), lin2.bias.detach().cpu().double()
    lg = x64 @ W64
    ext = x64 @ We64
    gates = torch.sigmoid(torch.relu(x64 @ W1.t() + b1) @ W2.t() + b2)
    two = torch.topk(lg, 2, dim=1)[0] if C > 1 else None
    sr = {"logits_top_classifier": lg, "logits_delta_softmax_classifier": lg.softmax(dim=1),
          "logits_delta_diff_classifier": (two[:, 0] - two[:, 1]).abs().unsqueeze(1).expand(-1, C),
          "logits_bottomk_irrel_classifier": ext[:, C:].max(dim=1)[0].unsqueeze(1).expand(-1, C)}
    return lg, ext, gates, O.mix_eval(gates, sr, discard)


@pytest.mark.parametrize("case", CASES, ids=[f"C{c[0]}-{c[1]}-D{c[2]}{'-discard' if c[6] else ''}" for c in CASES])
def test_patch_maps_exact_and_against_oracle(gpu_device, case):
    from moc_amd import engine, main_moc as M, patch_maps as PM
    dev = gpu_device
    C, st, D, sizes, j, K, discard, W, We, bags, labels, model, args = _setup(case, dev)
    res = M.ResidentBags(bags, labels, dev, dtype=DT[st])
    maps = PM.patch_maps(model, res, dev, args)
    assert len(maps) == len(sizes)

    # 2. pooled == the evaluation pass's logits, bit for bit
    pooled_eval, lab_eval, _ = M._eval_pass(res, dev, args, "eval", model=model)
    assert np.array_equal(np.stack([m.pooled for m in maps]), pooled_eval.numpy())
    assert [m.label for m in maps] == lab_eval == labels
    assert [m.pred for m in maps] == pooled_eval.argmax(dim=1).tolist()

    # 1. the dense gates / mixed at every union row == the prediction's own forward (keep_hidden: gates written)
    bank = M._bank_for(res.X, dev)
    batch = res.eval_plan(bank.C, bank.Ce, j, K, list(discard))["batch"]
    batch.phase_a(bank, for_eval=True)
    meta = engine.MetaState(model)
    engine.meta_forward(batch, meta, 0, batch.n_slides, engine.eval_use_bits(discard), keep_hidden=True)
    t, _ = batch.meta_ws()
    g_sel, m_sel = t["gates"].cpu().numpy(), t["mixed"].cpu().numpy()
    sel_idx, n_sel = batch.sel_idx.cpu().numpy(), batch.n_sel.cpu().numpy()
    for b, m in enumerate(maps):
        o, S = batch.row_off_host[b], int(n_sel[b])
        rows = sel_idx[o:o + S]
        assert np.array_equal(np.flatnonzero(m.selected), rows)
        assert np.array_equal(m.gates[rows], g_sel[o:o + S]), f"slide {b}: dense gates differ at union rows"
        assert np.array_equal(m.mixed[rows], m_sel[:, o:o + S].T), f"slide {b}: dense mixed differs at union rows"

    for b, m in enumerate(maps):
        N = sizes[b]
        assert m.coords.shape == (N, 2) and m.logits.shape == (N, C) and m.gates.shape == (N, 4)
        assert m.mixed.shape == (N, C) and m.selected.shape == (N,)
        S = int(m.selected.sum())
        assert m.evidence.shape == (C, min(K, S)) and m.zs_evidence.shape == (C, min(K, N))
        # 3. the evidence rows are what the pooled logit averages
        for c in range(C):
            mean = float(np.mean(m.mixed[m.evidence[c], c].astype(np.float64)))
            assert abs(mean - float(m.pooled[c])) <= 1e-6, (b, c, mean, m.pooled[c])
            assert m.selected[m.evidence[c]].all()
        # 4. float64 oracle on the stored (rounded) bag
        x64 = bags[b].to(DT[st]).double()
        lg, ext, gates, mixed = _oracle_rows(x64, W.double(), We.double(), model, C, discard)
        np.testing.assert_allclose(m.logits, lg.numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(m.gates, gates.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(m.mixed, mixed.numpy(), rtol=0, atol=2e-6)
        exp_sel = set(O.slide_process(x64, W.double(), We.double(), C, j, discard=discard)["selected_index"])
        amb = H.ambiguous_rows(H.selector_keys(ext, C), j)
        diff = set(np.flatnonzero(m.selected).tolist()) ^ exp_sel
        assert diff <= amb, f"slide {b}: union differs outside the tie band at {sorted(diff - amb)[:8]}"
        sel_rows = np.flatnonzero(m.selected)
        for c in range(C):
            key = mixed[:, c]
            kk = min(K, len(sel_rows))
            exp = sel_rows[torch.topk(key[sel_rows], kk)[1].numpy()]
            H.assert_topj_set(m.evidence[c], exp, key, what=f"evidence slide {b} class {c}")
            exp_zs = torch.topk(lg[:, c], min(K, N))[1].numpy()
            H.assert_topj_set(m.zs_evidence[c], exp_zs, lg[:, c], what=f"zs evidence slide {b} class {c}")


def test_zero_shot_maps_without_a_model(gpu_device):
    from moc_amd import engine, main_moc as M, patch_maps as PM
    dev = gpu_device
    C, st, D, sizes, j, K, discard, W, We, bags, labels, model, args = _setup(CASES[1], dev)
    res = M.ResidentBags(bags, labels, dev, dtype=DT[st])
    zs = PM.patch_maps(None, res, dev, args)
    full = PM.patch_maps(model, res, dev, args)
    for a, b in zip(zs, full):
        assert a.gates is None and a.mixed is None and a.evidence is None
        assert np.array_equal(a.logits, b.logits) and np.array_equal(a.zs_evidence, b.zs_evidence)
        assert np.array_equal(a.selected, b.selected)
    # the zero-shot pooled logits are topj_pooling's (zs_evaluation's)
    exp, _, _ = M._eval_pass(res, dev, args, "zs_topj")
    assert np.array_equal(np.stack([a.pooled for a in zs]), exp.numpy())


def _split_on_disk(root, bags, labels, seed):
    from moc_amd import datasets as DS
    data = os.path.join(root, "data")
    rng = np.random.default_rng(seed)
    ids, coords = [], []
    for i, b in enumerate(bags):
        sid = f"slide_{i:03d}"
        c = rng.integers(0, 200000, size=(b.shape[0], 2)).astype(np.int64)
        DS.write_bag(data, sid, b, coords=c, fmt="pt")
        ids.append(sid)
        coords.append(c)
    sp = DS.Generic_Split(pd.DataFrame({"slide_id": ids, "label": labels}), data_dir=data, num_classes=max(labels) + 1)
    sp.load_full_path(True)
    return sp, ids, coords


def test_coordinates_from_bag_files_resident_and_generic(gpu_device, tmp_path):
    from moc_amd import datasets as DS, patch_maps as PM
    dev = gpu_device
    C, st, D, sizes, j, K, discard, W, We, bags, labels, model, args = _setup(CASES[0], dev, seed=23)
    sp, ids, coords = _split_on_disk(str(tmp_path), bags, labels, 5)
    res = DS.to_resident(sp, dev)
    for k, c in enumerate(coords):
        assert np.array_equal(res.slide_coords[k], c)
    maps_res = PM.patch_maps(model, res, dev, args)
    loader = torch.utils.data.DataLoader(sp, batch_size=1, shuffle=False, num_workers=0)
    maps_gen = PM.patch_maps(model, loader, dev, args)
    for m, g, c, sid in zip(maps_res, maps_gen, coords, ids):
        assert np.array_equal(m.coords, c) and np.array_equal(g.coords, c)
        assert os.path.basename(m.path) == os.path.basename(g.path) == f"{sid}.pt"
        for f in ("pooled", "logits", "gates", "mixed", "selected", "evidence", "zs_evidence"):
            assert np.array_equal(getattr(m, f), getattr(g, f)), f
    PM.write_patch_maps(maps_res, str(tmp_path / "maps"))
    index = json.load(open(tmp_path / "maps" / "index.json"))
    assert list(index) == ids
    for m, c, sid in zip(maps_res, coords, ids):
        z = np.load(str(tmp_path / "maps" / index[sid]["file"]))
        assert np.array_equal(z["coords"], c)
        assert np.array_equal(z["evidence_coords"], c[m.evidence])
        assert np.array_equal(z["zs_evidence_coords"], c[m.zs_evidence])


def _driver_task(root, seed=31):
    """A two-class task in the driver's on-disk layout (dataset csv, 2-shot split, pt bags with coordinates, weights)."""
    from moc_amd import datasets as DS
    C = 2
    W, We = synth.make_bank(seed, 512, C)
    wdir = os.path.join(root, "models", "classifier_weights")
    os.makedirs(wdir, exist_ok=True)
    torch.save(W, os.path.join(wdir, "weights_nsclc_conch.pt"))
    torch.save(We, os.path.join(wdir, "weights_nsclc_ext_conch.pt"))
    data = os.path.join(root, "data", "nsclc", "merge_features_conch")
    names = ["LUAD", "LUSC"]
    rows, split = [], {}
    rng = np.random.default_rng(seed)
    for s_i, (key, n) in enumerate((("train", 4), ("val", 6), ("test", 4))):
        sizes = [int(v) for v in rng.integers(200, 900, size=n)]
        bags, labels = synth.make_slide_set(seed + 1000 * (s_i + 1), sizes, 512, We, C)
        ids = []
        for i, (b, y) in enumerate(zip(bags, labels)):
            sid = f"{key}_{i:02d}"
            DS.write_bag(data, sid, b, coords=rng.integers(0, 90000, size=(b.shape[0], 2)), fmt="pt")
            rows.append((f"p_{sid}", sid, names[y]))
            ids.append(sid)
        split[key] = pd.Series(ids)
    os.makedirs(os.path.join(root, "dataset_csv"), exist_ok=True)
    pd.DataFrame(rows, columns=["case_id", "slide_id", "label"]).to_csv(os.path.join(root, "dataset_csv", "nsclc.csv"), index=False)
    sdir = os.path.join(root, "splits", "nsclc_fewshot", "2shots")
    os.makedirs(sdir, exist_ok=True)
    pd.DataFrame(split).to_csv(os.path.join(sdir, "splits_0.csv"))
    return split["test"].tolist()


def test_driver_writes_maps_and_reproduces_them_from_the_checkpoint(gpu_device, tmp_path):
    from moc_amd import main_moc as M, patch_maps as PM, run_moc
    test_ids = _driver_task(str(tmp_path))
    common = ["--root", str(tmp_path), "--dataset", "nsclc", "--shot", "2", "--fold", "0", "--topj", "20", "--topk", "5",
              "--disable_tqdm", "--seed", "0"]
    res = run_moc.cli(common + ["--epochs", "2", "--result_dir", str(tmp_path / "res"), "--patch_maps", "test"])
    ckpt = res["best_model_path"]
    assert os.path.exists(ckpt)
    out1 = tmp_path / "res" / "patch_maps_shot_2_fold_0" / "test"
    assert sorted(os.listdir(out1)) == sorted([f"{s}.npz" for s in test_ids] + ["index.json"])
    index = json.load(open(out1 / "index.json"))
    assert list(index) == test_ids

    got = run_moc.cli(common + ["--result_dir", str(tmp_path / "inf"), "--patch_maps_from", ckpt])
    out2 = tmp_path / "inf" / "patch_maps_shot_2_fold_0" / "test"
    assert sorted(os.listdir(out2)) == sorted(os.listdir(out1))
    assert json.load(open(out2 / "index.json")) == index
    for s in test_ids:
        a, b = np.load(str(out1 / f"{s}.npz")), np.load(str(out2 / f"{s}.npz"))
        assert sorted(a.files) == sorted(b.files)
        for f in a.files:
            assert np.array_equal(a[f], b[f]), (s, f)
        m = PM.load_patch_map(str(out2 / f"{s}.npz"))
        assert m.gates is not None and m.evidence is not None and os.path.basename(m.path) == f"{s}.pt"
    assert not os.path.exists(tmp_path / "inf" / "zs_results_shot_2_fold_0.json")        # no zero-shot pass, no training
    on_disk = json.load(open(tmp_path / "inf" / "patch_maps_results_shot_2_fold_0.json"))
    assert on_disk == got and list(on_disk) == ["test"]

    # the results file is evaluation() of that checkpoint
    args = run_moc.get_args(common)
    dev = gpu_device
    _, _, te = run_moc.prepare(args, dev)
    model = M.senet(512, 4).to(dev)
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    exp = M.evaluation(model, te, dev, args)
    assert json.loads(json.dumps(exp)) == on_disk["test"]
