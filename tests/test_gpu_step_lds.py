"""The step kernels carve their dynamic LDS with the layouts of moc_amd/csrc/moc_step_lds.h.  These are the shapes at which
each layout's last arrays are used to their last byte -- where an off-by-one in a carve is wrong bits rather than a write
into padding: the narrow step at its largest LDS (60 pairs), with its row stage full (C K D = 20,480 floats) and with the
1,024-entry lists; the two forms of the three-launch step (pool_step_kernel + w1_update_kernel, topk_mean_kernel +
finish_kernel); the wide step in one chunk and in two, the second of eight pairs, which takes the zeroed slack rows behind
dz and the second trip through `region`.

The check is test_gpu_parity.py's test_gradient_only_step_matches_autograd, body and tolerance (helpers.grad_step_*):
moc_train_grad against autograd on the oracle, three slides of 700-900 rows, topj 40.  Every case first asserts that its
shape takes the kernel it is here for.  The narrow shapes run twice -- over the forward's tile records (a batch with a
mask of ones: pool_w1_step_tiles_kernel) and without (pool_w1_step_kernel) -- and the two runs agree bit for bit."""
import ctypes as C_

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

RECORDS, FULL = 1000001, 1000002      # MOC_TILE_PATH_RECORDS / MOC_TILE_PATH_FULL


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _mode(batch):
    from moc_amd._lib import lib
    return int(lib().moc_train_runs_mode(C_.byref(batch.c), C_.byref(batch.meta_ws()[1])))


def _supported(C, K, D):
    from moc_amd._lib import lib
    return int(lib().moc_p2p_step_supported(C, K, D, H.GRAD_STEP_TOPJ))


def _run(dev, C, K, D, dtype, tile_records):
    from moc_amd import engine as E
    keep = E.TILE_RECORDS
    E.TILE_RECORDS = tile_records
    try:
        batch, lab, meta = H.grad_step_batch(dev, C, K, D, dtype, masked=True)
        return _mode(batch), H.grad_step_grads(batch, lab, meta)
    finally:
        E.TILE_RECORDS = keep


# path: what the tile-record step leaves in n_pair[0] on each of the three slides.  With topj 40 the two-class slides have
# so few selected rows (a dozen tiles for the ten largest scores) that the records cannot prove exactness: on all three the
# kernel pools among the full scores instead, inside the same launch and the same layout -- MOC_TILE_PATH_FULL.
@pytest.mark.parametrize("C,K,D,dtype,path", [(15, 4, 256, torch.float32, RECORDS),     # narrow at its largest LDS: 60 pairs
                                              (2, 10, 1024, torch.float32, FULL),       # xs full: C K D = FS_MAX_XS
                                              (8, 7, 256, torch.bfloat16, RECORDS)])    # the 1,024-entry lists
def test_narrow_and_tile_record_steps_at_their_fullest(dev, C, K, D, dtype, path):
    assert _supported(C, K, D) == 1
    mode_n, narrow = _run(dev, C, K, D, dtype, False)
    mode_t, tiles = _run(dev, C, K, D, dtype, True)
    assert mode_n == 2 and mode_t == 1                            # one launch without records | over the tile records
    assert all(p == path for _, p in tiles) and all(p not in (RECORDS, FULL) for _, p in narrow)
    H.assert_grad_step_matches_autograd(narrow, C, K, D, dtype)
    H.assert_grad_step_matches_autograd(tiles, C, K, D, dtype)
    for (a, _), (b, _) in zip(narrow, tiles):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("C,K,D,dtype", [(8, 8, 256, torch.float32),        # 64 pairs, which narrow refuses: pool_step_kernel + w1_update_kernel
                                         (30, 10, 256, torch.bfloat16)])    # finish_kernel behind topk_mean_kernel
def test_three_launch_step(dev, C, K, D, dtype):
    assert _supported(C, K, D) == 0
    batch, lab, meta = H.grad_step_batch(dev, C, K, D, dtype)
    assert _mode(batch) == 0
    H.assert_grad_step_matches_autograd(H.grad_step_grads(batch, lab, meta), C, K, D, dtype)


@pytest.mark.parametrize("C,K,D,dtype", [(61, 8, 1024, torch.float32),      # 488 pairs, 480 per chunk: the last chunk is 8 pairs
                                         (30, 10, 512, torch.bfloat16)])    # one chunk
def test_wide_step_in_one_chunk_and_in_two(dev, C, K, D, dtype):
    assert _supported(C, K, D) == 1
    batch, lab, meta = H.grad_step_batch(dev, C, K, D, dtype)
    assert _mode(batch) == 2
    H.assert_grad_step_matches_autograd(H.grad_step_grads(batch, lab, meta), C, K, D, dtype)
