#!/usr/bin/env python3
"""Forward + backward of one ``make_chain()`` transition (256 x 256, 82 sub-steps) on its two gradient routes, alternating in one
process: ``grad='device'`` (the kernels of csrc/kflow.hip and their adjoint) and ``grad='torch'`` (torch autograd through the
torch-ops route), at batch 1 and batch 16.

    python tools/kflow_grad_bench.py [--out profiles/kflow_grad_bench.json]

A block is one forward + backward of each route, torch first; the figure is the median over 5 blocks after one warm-up of each
route, torch.cuda.synchronize() around every call, with the fastest and the slowest block recorded.  The peak device memory of a
route is ``torch.cuda.max_memory_allocated`` over one further forward + backward after ``reset_peak_memory_stats``, less what was
allocated before it (the input and the cotangent weights).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import chains  # noqa: E402
from sda_amd.experiments.kolmogorov import make_chain  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(args):
    routes = {'device': make_chain(grad='device'), 'torch': make_chain(grad='torch')}
    chain = routes['device']
    result = {'size': chain.size, 'dt': chain.dt, 'steps': chain.steps, 'blocks': args.blocks, 'device': torch.cuda.get_device_name(0),
              'cases': []}
    for batch in args.batches:
        x = chain.prior((batch,), device=args.device, seed=args.seed)
        w = torch.randn(x.shape, device=x.device, generator=torch.Generator(x.device).manual_seed(args.seed))

        def run(route):
            xs = x.clone().requires_grad_()
            (routes[route].transition(xs) * w).sum().backward()
            assert chains.LAST_KFLOW_GRAD_ROUTE == route
            return xs.grad

        grads = {r: run(r) for r in ('torch', 'device')}                  # warm-up of each route
        times = {'torch': [], 'device': []}
        for _ in range(args.blocks):
            for r in ('torch', 'device'):
                times[r].append(once(lambda: run(r))[0])
        peak = {}
        for r in ('torch', 'device'):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run(r)
            torch.cuda.synchronize()
            peak[r] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        ms = lambda ts: [round(t * 1e3, 3) for t in ts]                   # noqa: E731
        dm = statistics.median(times['device'])
        case = {'batch': batch}
        for r in ('device', 'torch'):
            case.update({f'{r}_ms': ms(times[r]), f'{r}_median_ms': round(statistics.median(times[r]) * 1e3, 3),
                         f'{r}_fastest_ms': round(min(times[r]) * 1e3, 3), f'{r}_slowest_ms': round(max(times[r]) * 1e3, 3),
                         f'{r}_peak_mib': peak[r]})
        case['device_median_below_fastest_torch_block'] = dm < min(times['torch'])
        case['max_abs_difference_of_the_gradients'] = float((grads['device'] - grads['torch']).abs().max())
        case['max_abs_gradient'] = float(grads['torch'].abs().max())
        result['cases'].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--device', default='cuda')
    p.add_argument('--out', default='profiles/kflow_grad_bench.json')
    main(p.parse_args())
