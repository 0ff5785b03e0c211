#!/usr/bin/env python3
"""Time ONE analysis of the ensemble-space smoother (csrc/enks_wide.hip: prepare, Gram, solve, transform) over a 9-slab window
against the same arithmetic in torch ops, float32 on the same device (the Gram products and the solve in float64 there too, as the
kernels do).  The observed values H are given (a component selection taken once, outside the timing): what is timed is the analysis.

  device   ops.enkw_prepare / enkw_gram / enkw_solve / enkw_transform
  torch    torch_analysis below
  fused    (Lorenz96(40) only) ops.enks_gain / enks_update, the observation-space kernels, on the same ensemble

Cases (M, d, k): (64, 8192, 512), (128, 8192, 2048), (64, 131072, 8192), and Lorenz96(40) at M = 128, k = 20.  The routes alternate
inside one process: a block times CALLS calls of one route, then of the next; reported are the median of 5 blocks (per call) with
the fastest and the slowest block, after one warm-up block.

    python tools/enks_wide_bench.py [--out profiles/enks_wide_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import ops  # noqa: E402

CALLS, BLOCKS, SLABS = 10, 5, 9
SHAPES = [('M64_d8192_k512', 64, 8192, 512), ('M128_d8192_k2048', 128, 8192, 2048), ('M64_d131072_k8192', 64, 131072, 8192),
          ('lorenz96_n40_M128_k20', 128, 40, 20)]


def torch_analysis(S, H, y, sigma, eps):
    m = H.shape[0]
    Y = H - H.double().mean(dim=0).float()
    D = (y + sigma * eps) - H
    Yd = Y.double()
    C = Yd @ Yd.T / (m - 1) + sigma ** 2 * torch.eye(m, device=H.device, dtype=torch.float64)
    W = torch.cholesky_solve(Yd @ D.double().T / (m - 1), torch.linalg.cholesky(C)).float()
    S += torch.matmul(W.T, S - S.mean(dim=1, keepdim=True))
    return S


def block(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def stats(ts):
    return {'median': round(statistics.median(ts), 4), 'fastest': round(min(ts), 4), 'slowest': round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/enks_wide_bench.json')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'calls_per_block': CALLS, 'blocks': BLOCKS, 'slabs': SLABS, 'sigma': 0.5,
              'unit': 'ms per analysis', 'cases': {}}
    sigma = 0.5
    for name, m, d, k in SHAPES:
        torch.manual_seed(0)
        S0 = torch.randn(SLABS, m, d, device=dev) + torch.randn(1, m, d, device=dev)
        index = torch.arange(k, device=dev) * (d // k)
        H = S0[-1][:, index].contiguous()
        y = H.mean(dim=0) + 0.3 * torch.randn(k, device=dev)
        eps = torch.randn(m, k, device=dev)
        S = S0.clone()
        Y, D, E = (torch.empty(m, k, device=dev) for _ in range(3))
        part = torch.empty(ops._lib.load().sda_enkw_gram_doubles(m, k), device=dev, dtype=torch.float64)
        work = torch.empty(m * m, device=dev, dtype=torch.float64)
        W = torch.empty(m, m, device=dev)
        status = torch.zeros(1, device=dev, dtype=torch.int32)

        def device():
            ops.enkw_prepare(H, y, sigma, seed=1, draw=0, Y=Y, D=D, eps=E)
            ops.enkw_gram(Y, D, part=part)
            ops.enkw_solve(part, m, k, sigma, W=W, status=status, work=work)
            ops.enkw_transform(S, 0, SLABS - 1, W)

        routes = {'device': device, 'torch': lambda: torch_analysis(S, H, y, sigma, eps)}
        if d <= 64 and k <= 64:
            o = ops.chain_obs(index.tolist(), [0.0] * k, [1.0] * k, sigma, y)
            a, z, wk = (torch.empty(k, m, device=dev) for _ in range(3))

            def fused():
                ops.enks_gain(S, SLABS - 1, o, seed=1, draw=0, a=a, z=z, work=wk, status=status)
                ops.enks_update(S, 0, SLABS - 1, a, z)
            routes['fused'] = fused
        times = {r: [] for r in routes}
        for r, fn in routes.items():                      # warm-up; every route starts a block from the same ensemble
            S.copy_(S0)
            block(fn)
        for _ in range(BLOCKS):
            for r, fn in routes.items():
                S.copy_(S0)
                times[r].append(block(fn))
        res = {'members': m, 'd': d, 'k': k, **{r + '_ms': stats(ts) for r, ts in times.items()}}
        res['device_median_below_torch_fastest'] = res['device_ms']['median'] < res['torch_ms']['fastest']
        result['cases'][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
