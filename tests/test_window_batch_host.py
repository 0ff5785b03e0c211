"""CPU: the index definition of the device-resident dataset (sda_window_batch_plan, csrc/dataset.hip: the kernel's own host/device index
functions; ops.window_batch_plan; sda_amd.data.DeviceTrajectories.index) against the numpy restatement tests/window_ref.py, the
properties a shuffled, windowed epoch must have, and the refusals of both entries without a GPU.  The device tests are
tests/test_gpu_window_batch.py and tests/test_gpu_graphed_feed.py."""
import ctypes

import numpy as np
import pytest
import torch

from sda_amd import _lib, data, ops
from sda_amd import build as sbuild
from tests import window_ref as R

BADARG, UNSUPPORTED = -1, -2
SEEDS = (0, 12345, 2 ** 32 + 7)
L, W = 11, 4
EPOCHS = 3


@pytest.fixture(scope='module')
def lib():
    sbuild.build()
    return _lib.load()


def _epochs(n, batch, seed, length=L, window=W, epochs=EPOCHS, first=0):
    """[(src_row, start)] per epoch from the C plan, every batch of the epoch concatenated in order (the last one short)."""
    spe = -(-n // batch)
    out = []
    for e in range(first, first + epochs):
        rows_, starts_ = [], []
        for i in range(spe):
            rows = min(batch, n - i * batch)
            src, st = ops.window_batch_plan(n, length, window, batch, seed, e * spe + i, rows)
            assert src.dtype == st.dtype == torch.int64 and src.shape == st.shape == (rows,)
            rows_.append(src.numpy())
            starts_.append(st.numpy())
        out.append((np.concatenate(rows_), np.concatenate(starts_)))
    return out


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n', [1, 2, 3, 5, 16, 17, 33, 1000])
def test_plan_equals_the_numpy_reference_and_every_epoch_is_a_permutation(lib, n, seed):
    """batch in {1, 4, N, N + 3}, three epochs (the first three, and for one batch size three that straddle step 2^32): rows and starts
    equal tests/window_ref.py exactly; every epoch's batches together hold each trajectory once (the short last batch completes the
    bijection); two epochs differ in order for N >= 5; starts lie in [0, L - W]."""
    for batch in (1, 4, n, n + 3):
        spe = -(-n // batch)
        first = (2 ** 32) // spe - 1 if batch == 4 else 0
        got = _epochs(n, batch, seed, first=first)
        for k, (src, st) in enumerate(got):
            e = first + k
            want_src = R.perm(np.arange(n), n, e, seed)
            s = e * spe + np.arange(n) // batch
            want_st = R.starts(L, W, s, np.arange(n) % batch, seed)
            assert np.array_equal(src, want_src), (batch, e)
            assert np.array_equal(st, want_st), (batch, e)
            assert np.array_equal(np.sort(src), np.arange(n)), (batch, e)
            assert st.min() >= 0 and st.max() <= L - W
        if n >= 5:
            assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[1][0], got[2][0])
    # the order of an epoch does not depend on how it is cut into batches
    assert np.array_equal(_epochs(n, 1, seed, epochs=1)[0][0], _epochs(n, n + 3, seed, epochs=1)[0][0])


def test_reference_plan_is_the_batch_slice_of_its_epoch():
    """window_ref.plan (what the device tests index with) == the slices used above."""
    n, batch, seed = 17, 4, SEEDS[2]
    for s in (0, 4, 9, 14):
        rows = min(batch, n - (s % 5) * batch)
        src, st = ops.window_batch_plan(n, L, W, batch, seed, s, rows)
        rs, rt = R.plan(n, L, W, batch, seed, s, rows)
        assert np.array_equal(src.numpy(), rs) and np.array_equal(st.numpy(), rt)


@pytest.mark.parametrize('seed', SEEDS)
def test_whole_trajectories_start_at_zero(lib, seed):
    for src, st in _epochs(9, 4, seed, length=6, window=6):
        assert not st.any()
    assert not R.starts(6, 6, np.arange(40)[:, None], np.arange(4)[None, :], seed).any()


SIGMA6 = 6 * np.sqrt(4096 * (1 / 8) * (7 / 8))          # 6 sigma of a Binomial(4096, 1/8) count: 127.0


def _assert_uniform(counts):
    assert counts.shape == (8,) and counts.sum() == 4096
    assert np.abs(counts - 512).max() <= SIGMA6, counts


@pytest.mark.parametrize('seed', SEEDS)
def test_starts_are_uniform(lib, seed):
    """4096 draws (64 batches of 64 rows) with L - W + 1 = 8: each start value's count within 6 sigma of 512 -- first in the numpy
    reference alone, then in the plan."""
    ref = R.starts(11, 4, np.arange(64)[:, None], np.arange(64)[None, :], seed).reshape(-1)
    _assert_uniform(np.bincount(ref, minlength=8))
    got = np.concatenate([ops.window_batch_plan(64, 11, 4, 64, seed, s, 64)[1].numpy() for s in range(64)])
    _assert_uniform(np.bincount(got, minlength=8))
    assert np.array_equal(got, ref)


@pytest.mark.parametrize('seed', SEEDS)
def test_shuffle_is_uniform(lib, seed):
    """N = 8 over 4096 epochs: every (position, trajectory) cell holds 512 +- 128 -- first in the numpy reference alone, then in the plan."""
    ref = R.perm(np.arange(8)[None, :], 8, np.arange(4096)[:, None], seed)

    def cells(orders):
        c = np.zeros((8, 8), dtype=np.int64)
        for p in range(8):
            c[p] = np.bincount(orders[:, p], minlength=8)
        return c
    c = cells(ref)
    assert (c.sum(0) == 4096).all() and (c.sum(1) == 4096).all() and np.abs(c - 512).max() <= 128, c
    got = np.stack([ops.window_batch_plan(8, 5, 2, 8, seed, e, 8)[0].numpy() for e in range(4096)])
    c = cells(got)
    assert np.abs(c - 512).max() <= 128, c
    assert np.array_equal(got, ref)


def test_bad_geometry_is_refused_without_a_gpu(lib):
    x, out = torch.zeros(5, 7, 3), torch.zeros(4, 6)
    src, st = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()

    def batch(dp=x.data_ptr(), n=5, length=7, f=3, w=2, b=4, rows=4, step=0, sd=None, op=out.data_ptr()):
        return lib.sda_window_batch(dp, n, length, f, w, b, rows, 7, step, sd, op, None)

    def plan(n=5, length=7, w=2, b=4, rows=4, step=0, sp=src, tp=st):
        return lib.sda_window_batch_plan(n, length, w, b, 7, step, rows, sp, tp)
    common = (dict(n=0), dict(n=-1), dict(length=0), dict(w=0), dict(w=8), dict(b=0), dict(rows=0), dict(rows=5), dict(step=-1),
              dict(step=1, rows=2),                # batch 1 of the epoch holds one trajectory (positions 4 .. 4)
              dict(step=3, rows=4))                # ... and so does batch 1 of the next epoch
    for kw in common:
        assert batch(**kw) == BADARG, kw
        assert plan(**kw) == BADARG, kw
    for kw in (dict(dp=None), dict(op=None), dict(f=0), dict(f=-4)):
        assert batch(**kw) == BADARG, kw
    for kw in (dict(sp=None), dict(tp=None)):
        assert plan(**kw) == BADARG, kw
    assert plan(step=1, rows=1) == 0 and plan(step=2, rows=4) == 0
    for kw in (dict(n=2 ** 31), dict(length=2 ** 31, w=1), dict(b=2 ** 31, rows=1)):
        assert batch(**kw) == UNSUPPORTED, kw
        assert plan(**kw) == UNSUPPORTED, kw
    assert batch(n=2 ** 31 - 1, b=2 ** 31 - 1, rows=2 ** 31 - 1, length=300, w=300, f=4) == UNSUPPORTED          # rows * 2 chunks
    assert batch(f=2 ** 42) == UNSUPPORTED                                                                        # chunks of one row
    assert batch(n=2 ** 30, length=2 ** 30, f=2 ** 10, b=4, rows=4) == UNSUPPORTED                                # N L F >= 2^63
    with pytest.raises(_lib.SdaHipError, match='CPU tensor'):
        ops.window_batch(x, 2, 4, 4, 7)


def test_device_trajectories_geometry_and_index_agree_with_the_plan(lib):
    """DeviceTrajectories on the host (device='cpu': no gather) -- len, steps_per_epoch, rows, remaining, the batch shapes and index."""
    x = np.arange(10 * 9 * 2 * 3, dtype=np.float64).reshape(10, 9, 2, 3)
    ds = data.DeviceTrajectories(x, window=4, flatten=True, seed=SEEDS[2], device='cpu')
    assert len(ds) == 10 and ds.data.dtype == torch.float32 and ds.data.is_contiguous()
    assert [ds.steps_per_epoch(b) for b in (1, 3, 4, 5, 10, 13)] == [10, 4, 3, 2, 1, 1]
    assert [ds.rows(4, s) for s in range(7)] == [4, 4, 2, 4, 4, 2, 4]
    assert ds.batch_shape(4) == (4, 8, 3)
    assert data.DeviceTrajectories(x, window=4, device='cpu').batch_shape(2) == (2, 4, 2, 3)
    assert data.DeviceTrajectories(x, device='cpu').batch_shape(2) == (2, 9, 2, 3)
    for s in range(7):
        src, st = ds.index(4, s)
        rs, rt = R.plan(10, 9, 4, 4, SEEDS[2], s, ds.rows(4, s))
        assert np.array_equal(src.numpy(), rs) and np.array_equal(st.numpy(), rt)
    assert ds.remaining(4) == 3
    ds.seek(4)
    assert ds.remaining(4) == 2 and ds.rows(4) == 4 and int(ds.cursor) == 4
    with pytest.raises(ValueError):
        ds.seek(-1)
    with pytest.raises(ValueError):
        data.DeviceTrajectories(x, window=10, device='cpu')
    with pytest.raises(ValueError):
        data.DeviceTrajectories(np.zeros((3, 4)), flatten=True, device='cpu')
    with pytest.raises(_lib.SdaHipError, match='CPU tensor'):
        ds.draw(4)


def test_from_h5_says_what_is_missing():
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='h5py'):
            data.DeviceTrajectories.from_h5('train.h5', window=5)
