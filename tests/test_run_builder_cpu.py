"""run_moc.build_run on the CPU: for each way a grid driver seeds its runs, the (meta-learner, Adam, mask generator) it
returns are those of the sequence the drivers used to spell out -- seed, `senet(FEATURE_DIM, 4)`, a private generator that
takes the default generator's state, Adam -- and two runs built from one seed are equal."""
import pytest
import torch

from moc_amd import main_moc as M
from moc_amd import run_moc

DEVICE = torch.device("cpu")


def _inline(seed, lr, weight_decay):
    """The sequence as cli_folds / cli_hgrid / cli_optgrid / cli_bankgrid each had it."""
    if seed is not None:
        torch.manual_seed(seed)
    model = M.senet(run_moc.FEATURE_DIM, 4).to(DEVICE)
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    return model, torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay), g


def _same(a, b):
    (ma, oa, ga), (mb, ob, gb) = a, b
    sa, sb = ma.state_dict(), mb.state_dict()
    assert list(sa) == list(sb) and len(sa) > 0
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(ga.get_state(), gb.get_state())
    assert len(oa.param_groups) == len(ob.param_groups) == 1
    assert {k: v for k, v in oa.param_groups[0].items() if k != "params"} == {k: v for k, v in ob.param_groups[0].items() if k != "params"}
    assert [id(p) for p in oa.param_groups[0]["params"]] == [id(p) for p in ma.parameters()]


# (how the driver seeds, seed, lr, weight decay): cli_folds / cli_hgrid without --seed go on from wherever the default stream
# is and with --seed start from it; cli_optgrid seeds with the cell's seed and builds Adam from the cell's rates; cli_bankgrid
# seeds with --seed
WAYS = [("no --seed", None, 1e-3, 1e-4), ("--seed", 3, 1e-3, 1e-4), ("a cell's seed and rates", 11, 3e-4, 0.0), ("--banks", 1, 2e-3, 1e-2)]


@pytest.mark.parametrize("way,seed,lr,wd", WAYS, ids=[w[0] for w in WAYS])
def test_the_builder_equals_the_inline_sequence(way, seed, lr, wd):
    torch.manual_seed(12345)                    # where "the stream is" when the run is built without a seed
    torch.rand(7)
    start = torch.get_rng_state()
    want = _inline(seed, lr, wd)
    left = torch.get_rng_state()
    torch.set_rng_state(start)
    got = run_moc.build_run(seed, DEVICE, lr=lr, weight_decay=wd)
    _same(got, want)
    assert torch.equal(torch.get_rng_state(), left)         # the default stream is left where the sequence left it
    assert got[1].param_groups[0]["lr"] == lr and got[1].param_groups[0]["weight_decay"] == wd
    # the generator starts where the constructor stopped: the masks follow the parameters in the stream
    assert torch.equal(got[2].get_state(), left)


def test_two_runs_from_one_seed_are_equal_and_unseeded_ones_are_not():
    a = run_moc.build_run(5, DEVICE, lr=1e-3, weight_decay=1e-4)
    torch.rand(3)                               # whatever happened in between
    b = run_moc.build_run(5, DEVICE, lr=1e-3, weight_decay=1e-4)
    _same(a, b)
    assert a[0] is not b[0] and a[2] is not b[2]
    assert torch.equal(torch.rand(4, generator=a[2]), torch.rand(4, generator=b[2]))
    # without a seed the second run goes on in the stream: other parameters, another generator state
    c = run_moc.build_run(None, DEVICE, lr=1e-3, weight_decay=1e-4)
    d = run_moc.build_run(None, DEVICE, lr=1e-3, weight_decay=1e-4)
    assert not all(torch.equal(x, y) for x, y in zip(c[0].state_dict().values(), d[0].state_dict().values()))
    assert not torch.equal(c[2].get_state(), d[2].get_state())
