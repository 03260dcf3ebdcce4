"""The pure parts the evaluation family shares (moc_amd.main_moc): the "visit every slide once" scope with its two
restore flavours, the accumulator that turns host chunks into metrics, the fused zero-shot column table -- and that
main_moc no longer reaches into the engine's privates."""
import os
import re

import pytest
import torch

import helpers as H
from moc_amd import main_moc as M


def _loader(repeat_num, n=5):
    return H.ListLoader([torch.zeros(1, 1)] * n, [0] * n, repeat_num)


# repeat_num before -> after the scope: "len" leaves len(dataset) (None and 0 become real_len), "attr" the attribute itself
@pytest.mark.parametrize("before", [None, 0, 8, 3])
def test_scope_sets_real_len_and_restores_in_its_flavour(before):
    for restore, after in (("len", before or 5), ("attr", before)):
        ld = _loader(before)
        assert torch.is_grad_enabled()
        with M._every_slide_once(ld, restore=restore) as real_len:
            assert real_len == 5 and ld.dataset.repeat_num == 5 and len(ld) == 5 and not torch.is_grad_enabled()
        assert ld.dataset.repeat_num == after and type(ld.dataset.repeat_num) is type(after) and torch.is_grad_enabled()
        assert len(ld.dataset) == (before or 5)


@pytest.mark.parametrize("restore", ["len", "attr"])
def test_scope_restores_on_an_exception(restore):
    ld = _loader(8)
    with pytest.raises(KeyError):
        with M._every_slide_once(ld, restore=restore):
            assert ld.dataset.repeat_num == 5
            raise KeyError("x")
    assert ld.dataset.repeat_num == 8 and torch.is_grad_enabled()
    with pytest.raises(AssertionError):
        with M._every_slide_once(ld, restore="both"):
            pass
    assert ld.dataset.repeat_num == 8


def test_scope_over_loaders_that_share_a_dataset_restores_last_first():
    a, b = _loader(None), _loader(9, n=4)
    again = H.ListLoader([], [])
    again.dataset = a.dataset                              # the first split named twice
    with M._every_slide_once(a, b, again) as real_len:
        assert real_len == 5 and a.dataset.repeat_num == 5 and b.dataset.repeat_num == 4
    # the second save of `a` saw real_len; restored last first, `a` ends at its FIRST-saved value: len() of a None split
    assert a.dataset.repeat_num == 5 and b.dataset.repeat_num == 9
    a.dataset.repeat_num = 7
    with M._every_slide_once(a, b, again):
        pass
    assert a.dataset.repeat_num == 7
    a.dataset.repeat_num = None
    with M._every_slide_once(a, again, restore="attr"):
        pass
    assert a.dataset.repeat_num is None


def _chunk(n, C, seed, slabs=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((slabs, n, C + 1) if slabs else (n, C + 1), generator=g)


def test_accumulator_rows_are_metrics_of_the_concatenation():
    args, C = H.make_args(3, 10, 10), 3
    ld = _loader(9, n=7)
    keys = ["b", "a", ("c", 1)]
    acc = M._Chunks(keys)
    assert list(acc.parts) == keys
    chunks = {k: [_chunk(n, C, 10 * i + j) for j, n in enumerate((3, 1, 3))] for i, k in enumerate(keys)}
    for j in range(3):
        for k in keys:
            acc.parts[k].append(chunks[k][j])
    acc.labels.extend([0, 1, 2, 0, 1, 2, 0])
    for k in keys:
        allv = torch.cat(chunks[k], 0)
        pooled, labels, losses = acc.rows(k)
        assert torch.equal(pooled, allv[:, :-1]) and pooled.is_contiguous() and labels is acc.labels and losses == allv[:, -1].tolist()
        want = M._metrics(allv[:, :-1].contiguous(), acc.labels, allv[:, -1].tolist(), 9, 7, args)
        got = acc.metrics(k, ld, 7, args)
        assert got == want and list(got) == ["loss", "acc", "auc"]
    # a subset of the rows (evaluation_runs: one run's slides)
    of = torch.tensor([5, 0, 2])
    allv = torch.cat(chunks["a"], 0)
    pooled, labels, losses = acc.rows("a", of=of)
    assert torch.equal(pooled, allv[of, :-1]) and labels == [2, 0, 2] and losses == allv[of, -1].tolist()
    assert list(acc.parts) == keys


def test_accumulator_slabs_give_one_metrics_dict_per_topk():
    args, C, n_k = H.make_args(2, 10, 10), 2, 3
    ld = _loader(None, n=6)
    keys = [(40, ()), (5, ("topk",))]
    acc = M._Chunks(keys, slabs=True)
    chunks = {k: [_chunk(n, C, 7 * i + j, slabs=n_k) for j, n in enumerate((2, 4))] for i, k in enumerate(keys)}
    for j in range(2):
        for k in keys:
            acc.parts[k].append(chunks[k][j])
    acc.labels.extend([0, 1, 0, 1, 0, 1])
    for k in keys:
        allv = torch.cat(chunks[k], 1)
        want = [M._metrics(allv[i, :, :-1].contiguous(), acc.labels, allv[i, :, -1].tolist(), 6, 6, args) for i in range(n_k)]
        assert acc.metrics(k, ld, 6, args) == want and len(want) == n_k
    assert list(acc.parts) == keys


def test_zs_columns_are_views_of_the_expected_rows():
    C = 3
    st = torch.arange((2 * C + 3) * 4, dtype=torch.float32).reshape(2 * C + 3, 4)
    want = {"topj": (slice(0, C), False, False), "delta_softmax": (slice(C, 2 * C), False, False),
            "delta_diff": (slice(2 * C, 2 * C + 1), False, True), "bottomk": (slice(2 * C + 1, 2 * C + 2), True, True)}
    assert sorted(M._ZS_KINDS.values()) == sorted(want) and tuple(M._ZS_KINDS) == M.ZS_POOLING_FUNCS
    for kind, (rows, small, shared) in want.items():
        keys, vals, s, sh = M._zs_columns(st, C, kind)
        assert (s, sh) == (small, shared)
        assert torch.equal(keys, st[rows]) and torch.equal(vals, st[:C])
        assert keys.data_ptr() == st[rows].data_ptr() and vals.data_ptr() == st.data_ptr()      # views, not copies


def test_main_moc_leaves_the_engines_privates_alone():
    src = open(os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "main_moc.py")).read()
    for private in ("._layout(", "._n_sel_stale("):
        assert private not in src, private
    assert not re.search(r"lib\(\)\s*\.\s*(moc_mask_compact|moc_scores|moc_ce_loss)\b", src)
    assert src.count("lib().moc_pool_loss") == 1            # _pool_loss_slabs: the copied workspace is its point
