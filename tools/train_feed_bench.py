"""ms per training EPOCH of ``utils.loop`` under two feeds, alternating block by block in ONE process:

  host     the reference's item recipe (sda/utils.py:76-86: ``from_numpy``, one ``randint``, one ``narrow``, one ``flatten`` per item),
           restated below, behind the shuffled ``DataLoader`` ``loop`` builds for any dataset object; ``loop`` uploads every batch
  device   ``sda_amd.data.DeviceTrajectories``: one gather launch per batch (csrc/dataset.hip), under ``graph=True`` inside the replayed step

Configurations, synthetic data 1024 x 1024 x 3 (the shape of the reference's Lorenz train.h5), batch 64, ``graph=True``: the Lorenz local
kernel (LOCAL_CONFIG on flattened windows of 5) and the Lorenz global net (64,) x (3,) on windows of 32 with ``net1d=True``.  Informational:
the Kolmogorov training net of tools/train_bench.py on 96 x 64 x 2 x 64 x 64, flattened windows of 5, batch 32, ``wgrad='tiled_ht'``, launch
by launch (its step is tens of ms: the feed is not expected to matter).

A block is ``--epochs`` consecutive epochs of one ``loop`` generator (training batches, a one-batch validation set, the epoch's loss read
back: wall clock around the block, which ends in that read-back and a device synchronise).  Per feed: the median of ``--blocks`` blocks,
the fastest and the slowest, as ms per epoch and per training step.  ``faster`` is true only where the device-fed median lies below the
host-fed route's FASTEST block.

    python tools/train_feed_bench.py --out profiles/train_feed_bench.json"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import Dataset  # noqa: E402

from sda_amd import utils  # noqa: E402
from sda_amd.data import DeviceTrajectories  # noqa: E402
from sda_amd.score import VPSDE  # noqa: E402


class HostTrajectories(Dataset):
    """The reference's TrajectoryDataset with an array for the file: the item recipe of sda/utils.py:76-86."""

    def __init__(self, data: np.ndarray, window: int = None, flatten: bool = False):
        self.data, self.window, self.flatten = data, window, flatten

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        x = torch.from_numpy(self.data[i])
        if self.window is not None:
            i = torch.randint(0, len(x) - self.window + 1, size=())
            x = torch.narrow(x, dim=0, start=i, length=self.window)
        if self.flatten:
            return x.flatten(0, 1), {}
        return x, {}


def configs(only):
    from sda_amd.experiments.kolmogorov import make_score
    from sda_amd.experiments.lorenz import make_global_score, make_local_score
    out = [
        dict(name='lorenz_local_b64', make=lambda: make_local_score().kernel, data=(1024, 1024, 3), window=5, flatten=True, shape=(15,),
             batch=64, loop=dict(graph=True), epochs=None, informational=False),
        dict(name='lorenz_global_b64', make=lambda: make_global_score(embedding=32, hidden_channels=(64,), hidden_blocks=(3,)),
             data=(1024, 1024, 3), window=32, flatten=False, shape=(32, 3), batch=64, loop=dict(graph=True, net1d=True), epochs=None,
             informational=False),
        dict(name='kolmogorov_b32', data=(96, 64, 2, 64, 64), window=5, flatten=True, shape=(10, 64, 64), batch=32,
             loop=dict(fused=True, wgrad='tiled_ht'), epochs=1, informational=True,
             make=lambda: make_score(window=5, embedding=64, hidden_channels=(96, 192, 384), hidden_blocks=(3, 3, 3), size=64).kernel),
    ]
    return [c for c in out if not only or c['name'] in only]


def feeds(cfg, dev, total_epochs):
    """{feed: a ``loop`` generator of ``total_epochs`` epochs} on two copies of one net over one array."""
    gen = torch.Generator().manual_seed(0)
    data = torch.randn(*cfg['data'], generator=gen)
    torch.manual_seed(0)
    base = cfg['make']()
    kw = dict(window=cfg['window'], flatten=cfg['flatten'])
    sets = {'host': (HostTrajectories(data.numpy(), **kw), HostTrajectories(data.numpy()[:cfg['batch']], **kw)),
            'device': (DeviceTrajectories(data, seed=0, device=dev, **kw), DeviceTrajectories(data[:cfg['batch']], seed=1, device=dev, **kw))}
    loops = {}
    for name, (train, valid) in sets.items():
        sde = VPSDE(copy.deepcopy(base), shape=cfg['shape']).to(dev)
        loops[name] = utils.loop(sde, train, valid, epochs=total_epochs, batch_size=cfg['batch'], learning_rate=1e-4, weight_decay=1e-3,
                                 device=dev, seed=0, **cfg['loop'])
    return loops


def block_ms(loop, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        triple = next(loop)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / epochs
    if not all(np.isfinite(triple)):
        raise RuntimeError(f'a non-finite epoch: {triple}')
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=32, help='epochs per block (the informational configuration runs 1)')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2, help='untimed epochs per feed')
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = dict(device=torch.cuda.get_device_name(dev), blocks=args.blocks, configs=[])
    for cfg in configs(args.only):
        epochs = cfg['epochs'] or args.epochs
        loops = feeds(cfg, dev, args.warmup + args.blocks * epochs)
        for loop in loops.values():
            for _ in range(args.warmup):
                next(loop)
        ms = {name: [] for name in loops}
        for _ in range(args.blocks):
            for name, loop in loops.items():
                ms[name].append(block_ms(loop, epochs))
        steps = -(-cfg['data'][0] // cfg['batch'])
        row = dict(name=cfg['name'], data=list(cfg['data']), window=cfg['window'], batch=cfg['batch'], loop=cfg['loop'],
                   steps_per_epoch=steps, epochs_per_block=epochs, informational=cfg['informational'])
        for name, v in ms.items():
            row[name] = dict(median_ms_per_epoch=round(statistics.median(v), 4), fastest_ms_per_epoch=round(min(v), 4),
                             slowest_ms_per_epoch=round(max(v), 4), median_ms_per_step=round(statistics.median(v) / steps, 4))
        row['faster'] = row['device']['median_ms_per_epoch'] < row['host']['fastest_ms_per_epoch']
        row['device_over_host'] = round(row['device']['median_ms_per_epoch'] / row['host']['median_ms_per_epoch'], 4)
        result['configs'].append(row)
        print(json.dumps(row), flush=True)
        del loops
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
