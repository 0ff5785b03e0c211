"""Device: the gather of the device-resident dataset (csrc/dataset.hip; ops.window_batch; sda_amd.data.DeviceTrajectories.draw).

The kernel contracts nothing -- it copies --, so every comparison is BITWISE against ``data[src_row, start:start + W]`` indexed on the
host from the plan (ops.window_batch_plan, pinned to the numpy definition by tests/test_window_batch_host.py)."""
import pytest
import torch

from sda_amd import data, ops

pytestmark = pytest.mark.gpu

SEED = 2 ** 32 + 11

# (N, L, F, W, batch): scalar path, short last batch, windows at odd element offsets | the 16-byte path | W F = 1028: a second chunk of four
# elements | W = L and F = 1 | a single trajectory | a frame shaped like Kolmogorov's (2, 8, 8)
SHAPES = [(5, 7, 3, 2, 4), (7, 9, 4, 3, 3), (3, 300, 4, 257, 2), (2, 6, 1, 6, 2), (1, 4, 8, 1, 1), (33, 5, 2 * 8 * 8, 5, 8)]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _data(n, length, f, gen_seed=0):
    """Distinct, exactly representable values: element (i, j, k) holds its own flat index (+ 1: never the 0 of a fresh buffer)."""
    return (torch.arange(n * length * f, dtype=torch.float32) + 1).view(n, length, f)


def _want(x, window, batch, s, rows, seed=SEED):
    src, st = ops.window_batch_plan(x.shape[0], x.shape[1], window, batch, seed, s, rows)
    return torch.stack([x[int(n), int(a):int(a) + window] for n, a in zip(src, st)])


def _steps(n, batch, epochs=2):
    spe = -(-n // batch)
    return [(s, min(batch, n - (s % spe) * batch)) for s in range(epochs * spe)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_batch_of_two_epochs_is_the_indexed_rows(dev, shape):
    n, length, f, window, batch = shape
    x = _data(n, length, f)
    xd = x.to(dev)
    for s, rows in _steps(n, batch):
        got = ops.window_batch(xd, window, batch, rows, SEED, step=s)
        assert got.shape == (rows, window, f)
        assert torch.equal(got.cpu(), _want(x, window, batch, s, rows)), s


@pytest.mark.parametrize('shape', [(5, 7, 3, 2, 4), (7, 9, 4, 3, 3), (3, 300, 4, 257, 2)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('offset', ['data', 'out'])
def test_views_offset_by_one_float_take_the_scalar_path_and_match(dev, shape, offset):
    """``data`` (or ``out``) one float into a larger allocation: 4-byte aligned only, so also F % 4 == 0 copies element by element."""
    n, length, f, window, batch = shape
    x = _data(n, length, f)
    big = torch.zeros(x.numel() + 8, device=dev)
    big[1:1 + x.numel()] = x.reshape(-1).to(dev)
    xd = big[1:1 + x.numel()].view(n, length, f) if offset == 'data' else x.to(dev)
    assert xd.data_ptr() % 16 == (4 if offset == 'data' else 0)
    for s, rows in _steps(n, batch, epochs=1):
        out = None
        if offset == 'out':
            out = torch.zeros(rows * window * f + 8, device=dev)[1:1 + rows * window * f]
            assert out.data_ptr() % 16 == 4
        got = ops.window_batch(xd, window, batch, rows, SEED, step=s, out=out)
        assert torch.equal(got.reshape(rows, window, f).cpu(), _want(x, window, batch, s, rows)), s


def test_device_counter_overrides_the_by_value_step_and_is_left_untouched(dev):
    n, length, f, window, batch = 5, 7, 3, 2, 4
    x = _data(n, length, f)
    xd = x.to(dev)
    counter = torch.tensor([2], device=dev, dtype=torch.int64)
    got = ops.window_batch(xd, window, batch, 4, SEED, step=99, step_dev=counter)          # (step 99 alone would be batch 1 of an epoch: 1 row)
    assert torch.equal(got.cpu(), _want(x, window, batch, 2, 4))
    assert not torch.equal(got[:1].cpu(), _want(x, window, batch, 99, 1))
    assert counter.item() == 2


def test_rows_past_the_epoch_end_are_left_unwritten(dev):
    """A full-batch launch at the device counter of a short batch (what a captured draw would do if replayed there): the rows inside the
    epoch are written, the others keep their content, nothing faults."""
    n, length, f, window, batch = 5, 7, 3, 2, 4
    x = _data(n, length, f)
    counter = torch.tensor([1], device=dev, dtype=torch.int64)
    out = torch.full((4, window, f), -7.0, device=dev)
    ops.window_batch(x.to(dev), window, batch, 4, SEED, step_dev=counter, out=out)
    assert torch.equal(out[:1].cpu(), _want(x, window, batch, 1, 1))
    assert (out[1:] == -7.0).all()


@pytest.mark.parametrize('shape', [(5, 7, 3, 2, 4), (7, 9, 4, 3, 3), (3, 300, 4, 257, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_guard_bands_stay_nan(dev, shape):
    n, length, f, window, batch = shape
    x = _data(n, length, f)
    xd = x.to(dev)
    guard = 64
    for s, rows in _steps(n, batch, epochs=1):
        numel = rows * window * f
        buf = torch.full((numel + 2 * guard,), float('nan'), device=dev)
        ops.window_batch(xd, window, batch, rows, SEED, step=s, out=buf[guard:guard + numel])
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + numel:]).all()
        assert torch.equal(buf[guard:guard + numel].view(rows, window, f).cpu(), _want(x, window, batch, s, rows))


def test_draw_iterates_epochs_and_flatten_shares_the_storage_layout(dev):
    """DeviceTrajectories over (N, L, 2, 3) frames: ``batches`` yields an epoch with its short last batch, ``flatten`` merges the first
    two item axes over identical storage, the cursor and its mirror advance together."""
    x = _data(10, 9, 6).view(10, 9, 2, 3)
    plain = data.DeviceTrajectories(x, window=4, seed=SEED, device=dev)
    flat = data.DeviceTrajectories(x, window=4, flatten=True, seed=SEED, device=dev)
    seen = []
    for epoch in range(2):
        got = list(plain.batches(4))
        assert [tuple(b.shape) for b, _kw in got] == [(4, 4, 2, 3), (4, 4, 2, 3), (2, 4, 2, 3)] and all(kw == {} for _b, kw in got)
        for i, ((b, _kw), (fb, _fkw)) in enumerate(zip(got, flat.batches(4))):
            s = epoch * 3 + i
            assert fb.shape == (b.shape[0], 8, 3) and fb.is_contiguous() and b.is_contiguous()
            assert torch.equal(fb.reshape(-1), b.reshape(-1))
            assert torch.equal(b.reshape(b.shape[0], 4, 6).cpu(), _want(x.view(10, 9, 6), 4, 4, s, b.shape[0]))
            seen.append(b)
    assert plain.cursor.item() == 6 and plain._s == 6 and plain.remaining(4) == 3
    whole = data.DeviceTrajectories(x, seed=SEED, device=dev).draw(10)
    assert whole.shape == (10, 9, 2, 3) and torch.equal(whole.cpu().sort(0).values, x.sort(0).values)


def test_captured_draw_replays_as_uncaptured_draws(dev):
    """``draw`` under torch.cuda.graph replayed three times == three uncaptured draws of a twin seeked to the same cursor."""
    x = _data(12, 9, 4)
    ds, twin = (data.DeviceTrajectories(x, window=3, seed=SEED, device=dev) for _ in range(2))
    ds.seek(3)
    twin.seek(3)
    static = torch.zeros(4, 3, 4, device=dev)
    ds.draw(4, out=static)                                    # (a first launch outside the capture; then back to the start)
    ds.seek(3)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds.draw(4, out=static)
    assert ds.cursor.item() == 3 and ds._s == 3               # (nothing ran)
    for k in range(3):
        graph.replay()
        ds.replayed()
        want = twin.draw(4)
        assert torch.equal(static, want), k
        assert torch.equal(want.cpu(), _want(x, 3, 4, 3 + k, 4))
    assert ds.cursor.item() == twin.cursor.item() == 6 and ds._s == twin._s == 6


def test_static_buffers_expect_full_batches(dev):
    ds = data.DeviceTrajectories(_data(5, 7, 3), window=2, seed=SEED, device=dev)
    ds.seek(1)
    with pytest.raises(ValueError, match='full batches'):
        ds.draw(4, out=torch.zeros(4, 2, 3, device=dev))
    assert ds.cursor.item() == 1 and ds.draw(4).shape == (1, 2, 3)
