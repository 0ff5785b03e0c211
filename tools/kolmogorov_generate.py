#!/usr/bin/env python3
"""Kolmogorov-flow training data on one device, by the protocol of the reference's experiments/kolmogorov/generate.py: per
trajectory ``prior``, 128 transitions of ``make_chain()`` (256 x 256, dt = 0.2), keep the last 64, ``coarsen(., 4)``.  The
trajectories are made in batches and split 80 / 10 / 10 into ``train.npy``, ``valid.npy`` and ``test.npy`` of shape
(N, 64, 2, 64, 64), which ``sda_amd.data.DeviceTrajectories(np.load(file), window=...)`` takes as they are (no HDF5: h5py is not
a dependency of this package).  Batch ``k`` draws its priors with ``seed + k``.

    python tools/kolmogorov_generate.py --trajectories 1024 --out data/kolmogorov
    python tools/kolmogorov_generate.py --bench [--bench-out profiles/kflow_bench.json]

``--bench`` times one transition of ``make_chain()`` on its two routes, alternating in one process: the kernels
(csrc/kflow.hip) and the same scheme in torch ops (``KolmogorovFlow._torch_transition``: torch.roll and torch.fft), at batch 1 and
batch 64.  A block is one transition of each route, torch first; the figure is the median over 5 blocks after one warm-up
transition of each route, torch.cuda.synchronize() around every call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd.experiments.kolmogorov import make_chain  # noqa: E402


def generate(args):
    chain = make_chain() if args.size is None else type(make_chain())(size=args.size, dt=0.2)
    n, done, parts = args.trajectories, 0, []
    t0 = time.perf_counter()
    k = 0
    while done < n:
        b = min(args.batch, n - done)
        x = chain.prior((b,), device=args.device, seed=args.seed + k)
        x = chain.trajectory(x, args.length - args.keep, last=True)
        x = chain.trajectory(x, args.keep)                               # (keep, b, 2, N, N)
        x = chain.coarsen(x, args.coarsen).transpose(0, 1)               # (b, keep, 2, N / r, N / r)
        parts.append(x.cpu().numpy())
        done += b
        k += 1
        print(f'{done} / {n} trajectories, {time.perf_counter() - t0:.1f} s', flush=True)
    x = np.concatenate(parts)
    if not np.isfinite(x).all():
        raise SystemExit('a trajectory is not finite')
    os.makedirs(args.out, exist_ok=True)
    i, j = int(0.8 * n), int(0.9 * n)
    for name, part in (('train', x[:i]), ('valid', x[i:j]), ('test', x[j:])):
        np.save(os.path.join(args.out, f'{name}.npy'), part)
        print(name, part.shape)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench(args):
    chain = make_chain()
    result = {'size': chain.size, 'dt': chain.dt, 'steps': chain.steps, 'blocks': args.blocks, 'device': torch.cuda.get_device_name(0),
              'cases': []}
    for batch in (1, 64):
        x = chain.prior((batch,), device=args.device, seed=args.seed)
        with torch.no_grad():
            ref = chain._torch_transition(x)                              # warm-up of each route
            got = chain.transition(x)
            kernel, torch_ms = [], []
            for _ in range(args.blocks):
                torch_ms.append(once(lambda: chain._torch_transition(x))[0])
                kernel.append(once(lambda: chain.transition(x))[0])
        ms = lambda ts: [round(t * 1e3, 3) for t in ts]                   # noqa: E731
        km = statistics.median(kernel)
        result['cases'].append({
            'batch': batch,
            'kernel_ms': ms(kernel), 'kernel_median_ms': round(km * 1e3, 3),
            'torch_ms': ms(torch_ms), 'torch_median_ms': round(statistics.median(torch_ms) * 1e3, 3),
            'torch_fastest_ms': round(min(torch_ms) * 1e3, 3),
            'kernel_median_below_fastest_torch_block': km < min(torch_ms),
            'kernel_ms_per_substep': round(km * 1e3 / chain.steps, 4),
            # generate.py's protocol: 128 transitions per trajectory
            'trajectories_per_hour_kernel': round(3600 * batch / (128 * km)),
            'trajectories_per_hour_torch': round(3600 * batch / (128 * statistics.median(torch_ms))),
            'max_abs_difference_of_the_routes': float((got - ref).abs().max()),
        })
        print(json.dumps(result['cases'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.bench_out)), exist_ok=True)
    with open(args.bench_out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--trajectories', type=int, default=1024)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--length', type=int, default=128)
    p.add_argument('--keep', type=int, default=64)
    p.add_argument('--coarsen', type=int, default=4)
    p.add_argument('--size', type=int, default=None, help='grid size (default: make_chain()\'s 256)')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--device', default='cuda')
    p.add_argument('--out', default='data/kolmogorov')
    p.add_argument('--bench', action='store_true')
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--bench-out', default='profiles/kflow_bench.json')
    a = p.parse_args()
    if a.bench:
        bench(a)
    else:
        generate(a)
