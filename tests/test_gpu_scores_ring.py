"""The score pass's LDS-DMA ring kernel (MOC_SCORES_RING, moc_scores_ring.hip) against the register-buffered streaming
kernel: the same registers into the same MFMAs in the same order and the same row epilogue, so EVERY output array is
compared bit for bit (int32 / uint8 views, poison included) -- there is no tolerance.  Needs an MI355X: run with -m gpu.

Both kernels write into buffers filled with NaN (statistics) and 0xFF (union flags) first: equal buffers then also say
that the ring kernel writes every slot the register kernel writes and nothing else; that kept slots hold numbers and
slots past a slide's kept rows keep the poison is asserted on its own."""
import ctypes as C

import pytest
import torch

from moc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _engine():
    from moc_amd import engine
    return engine


def _form(E, b):
    return E.lib().moc_scores_form(C.byref(b.c))


def _run(E, b, bank, ring):
    """scores() into poisoned buffers, twice (the second launch finds the LDS words of the first gone: nothing carries over)."""
    L = E._lib
    for _ in range(2):
        b.stats.fill_(float("nan"))
        b.sel_flag.fill_(255)
        if ring:
            b.c.flags |= L.MOC_SCORES_RING
        b.scores(bank)
    torch.cuda.synchronize()
    assert bool(b.c.flags & L.MOC_SCORES_RING) == ring
    return b.stats.clone(), b.sel_flag.clone(), (b.n_kept.clone() if b.n_kept is not None else None)


def _same_bits(E, X, sizes, Cn, bank, mask, x_starts=None, want_ring=True):
    L = E._lib
    outs = []
    for ring in (False, True):
        b = E.SlideBatch(X, sizes, Cn, Cn + 4, 10, 10, (), mask=mask, x_starts=x_starts)
        if ring:
            b.c.flags |= L.MOC_SCORES_RING
            assert (_form(E, b) == L.SCORE_FORM_RING) == want_ring, "the plan's choice for this shape"
        else:
            assert _form(E, b) != L.SCORE_FORM_RING
        outs.append(_run(E, b, bank, ring))
    (s0, f0, k0), (s1, f1, k1) = outs
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)), "statistics differ (or another set of slots was written)"
    assert torch.equal(f0, f1), "union flags differ"
    if k0 is not None:
        assert torch.equal(k0, k1)
    off = 0
    for i, n in enumerate(sizes):                           # every kept slot written, the rest of the slide untouched
        nk = int(k1[i]) if k1 is not None else n
        assert not torch.isnan(s1[:, off:off + nk]).any() and int(f1[off:off + nk].max() if nk else 0) == 0
        assert torch.isnan(s1[:, off + nk:off + n]).all() and (f1[off + nk:off + n] == 255).all()
        off += n


SIZES = [1, 15, 16, 17, 33, 300]        # partial last tiles, short first tiles (bases off multiples of 16), one whole tile


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("Cn", [2, 3])
def test_ring_kernel_gives_the_register_kernels_bits(dev, D, Cn):
    E = _engine()
    W, We = synth.make_bank(40 + Cn, D, Cn)
    bags, _ = synth.make_slide_set(500 + D + Cn, SIZES, D, We, Cn)
    X = torch.cat(bags).to(dev).contiguous()
    bank = E.Bank.get(W.to(dev), We.to(dev), torch.float32, dev)
    T = sum(SIZES)
    g = torch.Generator().manual_seed(5)
    half = (torch.rand(T, generator=g) > 0.5).to(torch.uint8)
    one = torch.zeros(T, dtype=torch.uint8)
    one[SIZES[0] + SIZES[1] + 7] = 1                       # one row of the whole batch: every other slide has no tile
    for mask in (None, half, torch.ones(T, dtype=torch.uint8), one):
        _same_bits(E, X, SIZES, Cn, bank, mask)


def test_ring_kernel_with_a_repeated_slide_in_the_visit_list(dev):
    E = _engine()
    D, Cn, bag_sizes = 256, 2, [300, 210]
    W, We = synth.make_bank(61, D, Cn)
    bags, _ = synth.make_slide_set(62, bag_sizes, D, We, Cn)
    X = torch.cat(bags).to(dev).contiguous()
    bank = E.Bank.get(W.to(dev), We.to(dev), torch.float32, dev)
    sizes, starts = [300, 210, 300], [0, 300, 0]
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(sum(sizes), generator=g) > 0.5).to(torch.uint8)
    for m in (None, mask):
        _same_bits(E, X, sizes, Cn, bank, m, x_starts=starts)


@pytest.mark.parametrize("D,N", [(256, 20011), (512, 20011), (256, 40)])
def test_ring_slots_wrap_and_idle_workgroups_end(dev, D, N):
    """20,011 rows: 1,251 tiles over 256 workgroups of four (D = 256: one unit a tile) or three (D = 512: two units a tile)
    slots -- every workgroup goes round its ring; 40 rows: three tiles, fewer than the launch's workgroups."""
    E = _engine()
    Cn = 2
    W, We = synth.make_bank(71, D, Cn)
    X = synth.make_bag(72 + D, N, D, We, Cn, label=1).to(dev).contiguous()
    bank = E.Bank.get(W.to(dev), We.to(dev), torch.float32, dev)
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(N, generator=g) > 0.5).to(torch.uint8)
    for m in (None, mask):
        _same_bits(E, X, [N], Cn, bank, m)


@pytest.mark.parametrize("D", [256, 512])
def test_ring_kernel_over_more_than_64_slides_with_empty_ones(dev, D):
    """150 slides of 1 ... 40 rows (production batches have hundreds): the tile prefix scan carries across its 64-slide
    chunks, and under a half mask that leaves some slides without a kept row the loader gallops over empty slides."""
    E = _engine()
    Cn, n = 2, 150
    g = torch.Generator().manual_seed(8)
    sizes = torch.randint(1, 41, (n,), generator=g).tolist()
    sizes[:6] = [1, 1, 2, 40, 1, 1]
    W, We = synth.make_bank(101, D, Cn)
    X = synth.make_bag(102 + D, sum(sizes), D, We, Cn, label=0).to(dev).contiguous()
    bank = E.Bank.get(W.to(dev), We.to(dev), torch.float32, dev)
    half = (torch.rand(sum(sizes), generator=g) > 0.5).to(torch.uint8)
    half[0] = 1                                                     # (the first slide keeps its row)
    off, empty = 0, []
    for i, s in enumerate(sizes):
        if int(half[off:off + s].sum()) == 0:
            empty.append(i)
        off += s
    assert len(empty) >= 3 and any(i >= 64 for i in empty) and any(i < 64 for i in empty), "slides without a kept row, in several chunks"
    for mask in (None, half):
        _same_bits(E, X, sizes, Cn, bank, mask)


def test_shapes_the_ring_kernel_does_not_cover_keep_their_kernels(dev):
    """16-bit bags and banks of more than one n-tile: the bit is accepted and the batch takes the kernel it always took."""
    E = _engine()
    L = E._lib
    D, sizes = 256, [300, 17]
    for dtype, Cn in ((torch.bfloat16, 2), (torch.float32, 60)):          # (60 classes + 4: four n-tiles)
        W, We = synth.make_bank(81 + Cn, D, Cn)
        bags, _ = synth.make_slide_set(82 + Cn, sizes, D, We, Cn)
        X = torch.cat(bags).to(dev).to(dtype).contiguous()
        bank = E.Bank.get(W.to(dev), We.to(dev), dtype, dev)
        b = E.SlideBatch(X, sizes, Cn, Cn + 4, 10, 10, ())
        b.c.flags |= L.MOC_SCORES_RING
        assert _form(E, b) == 0, "the streaming form"
        assert not b.use_score_ring() and not (b.c.flags & L.MOC_SCORES_RING)
        _same_bits(E, X, sizes, Cn, bank, None, want_ring=False)


def test_ring_bit_beside_a_ticket_is_refused(dev):
    E = _engine()
    L = E._lib
    D, Cn, sizes = 256, 2, [300, 17]
    W, We = synth.make_bank(91, D, Cn)
    bags, _ = synth.make_slide_set(92, sizes, D, We, Cn)
    X = torch.cat(bags).to(dev).contiguous()
    bank = E.Bank.get(W.to(dev), We.to(dev), torch.float32, dev)
    b = E.SlideBatch(X, sizes, Cn, Cn + 4, 10, 10, ())
    b.reserve_cus(0, ticket=True)
    b.c.flags |= L.MOC_SCORES_RING
    assert _form(E, b) < 0 and b"MOC_SCORES_RING takes neither tile_ticket nor cu_reserved" in E.lib().moc_last_error()
    with pytest.raises(AssertionError, match="MOC_SCORES_RING takes neither tile_ticket nor cu_reserved"):
        b.scores(bank)
    torch.cuda.synchronize()
    assert b.use_score_ring() and b.c.tile_ticket is None           # (use_score_ring drops the ticket)
