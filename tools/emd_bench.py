#!/usr/bin/env python3
"""Time metrics.emd on its two routes, alternating in one process:

  host     emd(solver='host'): cost matrix on the device, copied to the host, exact O(n^3) solve on one host thread
  device   emd(solver='device'): cost matrix and epsilon-scaling auction on the device (csrc/assign.hip), one record read back

Inputs: two independent sets of n trajectories of shape (65, 3) -- Gaussian clouds and, at n = 1024 where the chain kernels
load, two posterior() draws as experiments/lorenz/eval.py:58-59 makes them.  n = 1024 is the evaluation's size; 256 and 4096 are
timed on Gaussian clouds as well (fewer blocks at 4096, where one host solve takes seconds).  A block is one call of each
route, host first; the figure is the median over the blocks after one warm-up call of each route, torch.cuda.synchronize()
around every call.  Writes one JSON file with both medians, the fastest and slowest block, bids and gap of the device solve,
the shader clock, and the time a launch that spends the whole default bid budget at n = 4096 would take (extrapolated from
the time per bid of the n = 4096 solve: no input here needs the whole budget).

    python tools/emd_bench.py [--out profiles/emd_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import metrics, ops  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def compare(x, y, blocks):
    host, device = [], []
    ref = metrics.emd(x, y, solver='host')                   # warm-up of each route
    got = metrics.emd(x, y, solver='device')
    route = metrics.LAST_EMD_ROUTE
    for _ in range(blocks):
        host.append(once(lambda: metrics.emd(x, y, solver='host'))[0])
        device.append(once(lambda: metrics.emd(x, y, solver='device'))[0])
    n = x.shape[0]
    cost = ops.pairwise_dist(x.flatten(1).float(), y.flatten(1).float(), squared=False)
    solve_ms, res = once(lambda: ops.assignment_auction(cost, eps_rel=metrics.EMD_EPS_REL))
    ms = lambda ts: [round(t * 1e3, 3) for t in ts]          # noqa: E731
    return {
        'n': n, 'blocks': blocks, 'device_route': route,
        'emd_host': float(ref), 'emd_device': float(got),
        'host_ms': ms(host), 'host_median_ms': round(statistics.median(host) * 1e3, 3), 'host_fastest_ms': round(min(host) * 1e3, 3),
        'host_slowest_ms': round(max(host) * 1e3, 3),
        'device_ms': ms(device), 'device_median_ms': round(statistics.median(device) * 1e3, 3),
        'device_fastest_ms': round(min(device) * 1e3, 3), 'device_slowest_ms': round(max(device) * 1e3, 3),
        'device_faster_than_fastest_host_block': statistics.median(device) < min(host),
        'auction_launch_ms': round(solve_ms * 1e3, 3), 'bids': int(res.bids), 'bids_per_row': round(int(res.bids) / n, 2),
        'gap': float(res.gap), 'eps_final': float(res.eps_final), 'status': int(res.status),
        'bid_budget': ops.auction_default_budget(n),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/emd_bench.json')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--blocks-large', type=int, default=2, help='blocks at n = 4096 (one host solve takes seconds)')
    ap.add_argument('--sizes', type=int, nargs='*', default=[1024, 256, 4096])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'eps_rel': metrics.EMD_EPS_REL, 'clock_before': ops.clock_probe(dev), 'runs': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for n in args.sizes:
        x = torch.randn(n, 65, 3, device=dev, generator=g)
        y = torch.randn(n, 65, 3, device=dev, generator=g)
        result['runs'][f'gauss{n}'] = compare(x, y, args.blocks if n <= 1024 else args.blocks_large)
        print(json.dumps({f'gauss{n}': result['runs'][f'gauss{n}']}), flush=True)
    try:                                                     # two posterior() draws, as eval.py:58-59 ('hi' setting: 65 observations)
        from sda_amd import chains
        from sda_amd.experiments import lorenz
        chain = lorenz.make_chain()
        A = lambda x: chains.Lorenz63.preprocess(x)[..., :1]      # noqa: E731
        torch.manual_seed(0)
        truth = chain.trajectory(chain.trajectory(chain.prior((), device=dev), 64, last=True), 65)
        yobs = torch.normal(A(truth), 0.25)
        x = lorenz.posterior(yobs, A=A, sigma=0.25, step=1)[:1024]
        x_ = lorenz.posterior(yobs, A=A, sigma=0.25, step=1)[:1024]
        result['runs']['posterior1024'] = compare(x, x_, args.blocks)
        print(json.dumps({'posterior1024': result['runs']['posterior1024']}), flush=True)
    except Exception as e:                                   # the chain kernels are not what this tool measures
        result['posterior_skipped'] = repr(e)
    big = result['runs'].get('gauss4096')
    if big and big['bids']:
        result['budget_exhausted_launch_ms_at_4096_extrapolated'] = round(big['auction_launch_ms'] * big['bid_budget'] / big['bids'], 1)
    result['clock_after'] = ops.clock_probe(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
