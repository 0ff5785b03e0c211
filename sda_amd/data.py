r"""The training set on the device: shuffled, randomly windowed batches in one launch each (csrc/dataset.hip).

The reference feeds its training loop from ``TrajectoryDataset`` (sda/utils.py:58-86) behind a shuffled ``DataLoader``: per ITEM one
``torch.randint``, one ``narrow`` and one ``flatten`` on the host, then collation and an upload.  Since a replayed training step
(``training.GraphedStep``) costs a fraction of a millisecond, that feed is the slower half of an epoch.  The reference's training sets are
small (Lorenz 12 MB, Kolmogorov under 2 GB of fp32), so :class:`DeviceTrajectories` keeps the whole array on the device and gathers a
batch with ``ops.window_batch``::

    ds = sda_amd.data.DeviceTrajectories(x, window=5, flatten=True, seed=0)      # x: (N, L, *frame), tensor or numpy array
    for x, kwargs in ds.batches(64):                                            # one epoch, the last batch short
        ...
    for losses in sda_amd.utils.loop(sde, ds, ds_valid, graph=True, device='cuda'):  # the gather is the graph's first node
        ...

The order of an epoch and the window of every row are KEYED, as the loss noise of ``training.KeyedLossNoise`` is: row ``b`` of global
batch ``s`` (epoch ``s // steps_per_epoch``) is ``x[n_b, start_b:start_b + window]`` with ``(n_b, start_b)`` a function of
``(seed, s, b)`` alone -- a stateless permutation of the trajectories per epoch, a uniform first frame per row; ``index`` returns them on
the host.  They are not torch's generator stream.  ``s`` lives in a device int64 scalar (``cursor``), so ``draw`` can be captured in a
hipGraph and replayed.  Items carry no ``kwargs`` (weights or context per item are not served) and the set lives on one device."""
from typing import Iterator, Tuple

import torch
from torch import Tensor

from . import ops


class DeviceTrajectories:
    r"""``TrajectoryDataset`` with an array for the file, resident on ``device``.

    ``x``: a tensor or numpy array ``(N, L, *frame)``, converted once to contiguous fp32 on ``device``.  ``window=None``: whole
    trajectories (``W = L``).  Batches are ``(rows, W, *frame)``, with ``flatten=True`` ``(rows, W * frame[0], *frame[1:])`` -- what the
    reference's items collate to; both are views of one contiguous buffer.  ``seed`` keys the shuffle and the windows.

    ``device='cpu'`` keeps the array on the host: ``len``, ``steps_per_epoch`` and ``index`` work, ``draw`` refuses (there is no CPU
    gather)."""

    def __init__(self, x, window: int = None, flatten: bool = False, seed: int = 0, device='cuda'):
        x = torch.as_tensor(x)
        if x.dim() < 2 or x.numel() == 0:
            raise ValueError(f'DeviceTrajectories: x is (N, L, *frame) with at least one element (got {tuple(x.shape)})')
        if flatten and x.dim() < 3:
            raise ValueError('DeviceTrajectories: flatten=True merges the frame axis with the first item axis: x needs one')
        self.data = x.to(device=device, dtype=torch.float32).contiguous()
        self.length = int(x.shape[1])
        self.window = self.length if window is None else int(window)
        if not 1 <= self.window <= self.length:
            raise ValueError(f'DeviceTrajectories: 1 <= window <= L = {self.length} (got {window})')
        self.flatten, self.seed = bool(flatten), int(seed)
        self.cursor = torch.zeros(1, device=self.data.device, dtype=torch.int64)        # the global batch index s
        self._s = 0                                                                     # its host mirror

    @classmethod
    def from_h5(cls, file, window: int = None, flatten: bool = False, seed: int = 0, device='cuda') -> 'DeviceTrajectories':
        """The reference's constructor: dataset ``'x'`` of the HDF5 ``file`` (sda/utils.py:67-68).  Needs ``h5py``; this path is NOT
        covered by the test suite (h5py is not part of the build environment)."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError('DeviceTrajectories.from_h5 reads the file with h5py, which is not installed; load the array by other '
                              'means and pass it to DeviceTrajectories(x, ...)') from e
        with h5py.File(file, mode='r') as f:
            x = f['x'][:]
        return cls(x, window=window, flatten=flatten, seed=seed, device=device)

    # ------------------------------------------------------------------ geometry
    def __len__(self) -> int:
        return self.data.shape[0]

    def steps_per_epoch(self, batch_size: int) -> int:
        if batch_size < 1:
            raise ValueError('DeviceTrajectories: batch_size >= 1')
        return -(-len(self) // batch_size)

    def rows(self, batch_size: int, s: int = None) -> int:
        """Rows of global batch ``s`` (default: the next one): ``batch_size`` but for an epoch's last batch."""
        s = self._s if s is None else s
        return min(batch_size, len(self) - (s % self.steps_per_epoch(batch_size)) * batch_size)

    def remaining(self, batch_size: int) -> int:
        """Batches from the cursor to the end of its epoch."""
        spe = self.steps_per_epoch(batch_size)
        return spe - self._s % spe

    def batch_shape(self, rows: int) -> Tuple[int, ...]:
        frame = tuple(self.data.shape[2:])
        if self.flatten:
            return (rows, self.window * frame[0]) + frame[1:]
        return (rows, self.window) + frame

    def index(self, batch_size: int, s: int):
        """Host: ``(src_row, start)`` int64 CPU tensors of global batch ``s`` -- row ``b`` is ``x[src_row[b], start[b]:start[b] + window]``
        (ops.window_batch_plan: the kernel's own index functions; needs no GPU)."""
        return ops.window_batch_plan(len(self), self.length, self.window, batch_size, self.seed, s, self.rows(batch_size, s))

    # ------------------------------------------------------------------ the cursor
    def seek(self, s: int) -> None:
        """Set the global batch index (device scalar and host mirror)."""
        if s < 0:
            raise ValueError('DeviceTrajectories: seek(s >= 0)')
        self.cursor.fill_(int(s))
        self._s = int(s)

    def replayed(self, n: int = 1) -> None:
        """Tell the host mirror that a captured ``draw`` was replayed ``n`` times (a replay advances the device cursor only)."""
        self._s += int(n)

    # ------------------------------------------------------------------ batches
    def draw(self, batch_size: int, out: Tensor = None) -> Tensor:
        """The next batch: one ``ops.window_batch`` launch reading the device cursor, then ``cursor += 1`` on the device.  Capturable.
        With ``out`` (a contiguous fp32 device tensor of a full batch's elements) it fills that static buffer and expects a full batch.
        Under stream capture nothing runs, so the host mirror stays put: whoever replays the graph calls ``replayed()`` after each
        replay, and replays it at full batches only (at a short one the rows past the epoch's end would be left unwritten)."""
        capturing = self.data.is_cuda and torch.cuda.is_current_stream_capturing()
        rows = batch_size if capturing else self.rows(batch_size)          # (a capture runs nothing: the mirror says nothing about its replays)
        if rows > len(self) or (out is not None and rows != batch_size):
            raise ValueError(f'DeviceTrajectories.draw: a static buffer expects full batches of {batch_size} rows (N = {len(self)}, '
                             f'batch {self._s} has {self.rows(batch_size)})')
        got = ops.window_batch(self.data, self.window, batch_size, rows, self.seed, step=self._s, step_dev=self.cursor, out=out)
        self.cursor += 1
        if not capturing:
            self._s += 1
        return got.view(self.batch_shape(rows))

    def batches(self, batch_size: int) -> Iterator[Tuple[Tensor, dict]]:
        """One epoch from the current cursor as ``(x, {})`` pairs (the empty dict is the reference items' ``kwargs``), the last one short."""
        for _ in range(self.remaining(batch_size)):
            yield self.draw(batch_size), {}
