#!/usr/bin/env python3
"""Time the ensemble Kalman smoother (chains.enks_fused: per observation one forecast, one gain and one update launch) against the
same five steps of every analysis written in torch ops, float32 on the same device.  Both routes forecast with the chain kernels;
what differs is the analysis.

  device   sda_amd.chains.enks_fused
  torch    torch_enks below: mean / anomalies / covariance / torch.linalg.cholesky + cholesky_solve / two matmuls per analysis

Cases: M = 1024 and 16 384 on the 65 x 3 Lorenz-63 evaluation case ('lo': sigma 0.05, step 8, 9 observations; 'hi': sigma 0.25,
step 1, 65 observations; component 0 observed through preprocess), and M = 1024 on Lorenz96(n=40) observing every other component
(sigma 0.5, step 2, 16 observations).  The two routes alternate inside one process: a block times CALLS calls of one route, then of
the other; reported are the median of 5 blocks (per call) with the fastest and the slowest block, after one warm-up block, and
whether the device median lies below the torch route's FASTEST block.

    python tools/enks_bench.py [--out profiles/enks_bench.json]
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
from sda_amd.experiments import lorenz  # noqa: E402

CALLS, BLOCKS = 3, 5


def torch_enks(chain, x, y, obs, sigma, step, seed):
    """chains.enks_fused(lag=None, inflation=1) with every analysis in torch ops (float32, on x's device)."""
    m, d = x.shape
    n = len(y)
    index = torch.tensor(obs.index, device=x.device)
    shift, scale = x.new_tensor(obs.shift), x.new_tensor(obs.scale)
    k = len(obs.index)
    eye = torch.eye(k, device=x.device)
    gen = torch.Generator(device=x.device).manual_seed(seed)
    S = torch.empty(n * step + 1, m, d, device=x.device)
    S[0] = x
    for i in range(n):
        t = (i + 1) * step
        S[i * step + 1:t + 1] = chain.trajectory(S[i * step], step)
        h = (S[t][:, index] - shift) / scale
        a = h - h.mean(dim=0)
        C = a.T @ a / (m - 1) + sigma ** 2 * eye
        eps = torch.randn(m, k, device=x.device, generator=gen)
        z = torch.cholesky_solve(((y[i] + sigma * eps) - h).T, torch.linalg.cholesky(C)).T
        W = S[:t + 1]
        P = torch.einsum('smd,mk->sdk', W - W.mean(dim=1, keepdim=True), a) / (m - 1)
        W += torch.einsum('mk,sdk->smd', z, P)
    return S.permute(1, 0, 2).contiguous()


def block(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def cases(dev):
    l63 = lorenz.make_chain()
    o63 = chains.probe_affine(lambda x: l63.preprocess(x)[..., :1], l63, 3)
    for name, s in (('lo', dict(sigma=0.05, step=8, nobs=9)), ('hi', dict(sigma=0.25, step=1, nobs=65))):
        for m in (1024, 16384):
            yield f'lorenz63_{name}_M{m}', lorenz.make_chain(), o63, m, s
    yield 'lorenz96_n40_M1024', chains.Lorenz96(n=40), chains.AffineObservation(range(0, 40, 2), [0.0] * 20, [1.0] * 20), 1024, \
        dict(sigma=0.5, step=2, nobs=16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/enks_bench.json')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'calls_per_block': CALLS, 'blocks': BLOCKS, 'unit': 'ms per call', 'cases': {}}
    for name, chain, obs, m, s in cases(dev):
        torch.manual_seed(0)
        x0 = chain.trajectory(chain.prior((m,), device=dev), 64, last=True)
        truth = chain.trajectory(x0[:1], s['nobs'] * s['step'])[s['step'] - 1::s['step'], 0]
        y = torch.normal(obs(truth), s['sigma'])
        device = lambda: chains.enks_fused(chain, x0, y, obs, s['sigma'], s['step'], seed=1)      # noqa: E731
        plain = lambda: torch_enks(chain, x0, y, obs, s['sigma'], s['step'], 1)                  # noqa: E731
        block(device), block(plain)                                                             # warm-up
        td, tt = [], []
        for _ in range(BLOCKS):
            td.append(block(device))
            tt.append(block(plain))
        r = {**s, 'members': m, 'd': x0.shape[1], 'k': len(obs.index),
             'device_ms': {'median': round(statistics.median(td), 3), 'fastest': round(min(td), 3), 'slowest': round(max(td), 3)},
             'torch_ms': {'median': round(statistics.median(tt), 3), 'fastest': round(min(tt), 3), 'slowest': round(max(tt), 3)}}
        r['device_median_below_torch_fastest'] = r['device_ms']['median'] < r['torch_ms']['fastest']
        result['cases'][name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
