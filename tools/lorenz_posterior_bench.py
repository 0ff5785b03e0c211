#!/usr/bin/env python3
"""Time the particle-filter ground truth of the Lorenz evaluation (experiments/lorenz/eval.py:44-68) at 16 384 particles, for
both of its settings, on two routes:

  fused    sda_amd.experiments.lorenz.posterior(fused=True): one advance(+weights) / cdf / resample launch per observation
  torch    posterior's generic route with a torch-ops RK4 transition on the same device -- what a user had to write before the
           chain kernels existed (metrics.bpf around DiscreteODE.rk4 and Normal.sample)

Median of 5 timed calls after 2 warm-ups, torch.cuda.synchronize() around each call.  Writes one JSON file.

    python tools/lorenz_posterior_bench.py [--out profiles/chain_posterior_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import chains, metrics  # noqa: E402
from sda_amd.experiments import lorenz  # noqa: E402

SETTINGS = {'lo': dict(sigma=0.05, step=8, nobs=9), 'hi': dict(sigma=0.25, step=1, nobs=65)}


def torch_route(y, A, sigma, step, particles, device):
    """The reference's posterior() with every chain operation as torch ops on the device."""
    chain = lorenz.make_chain()

    def transition(x):
        return torch.distributions.Normal(chain._rk4_transition(x), chain.dt ** 0.5).sample()

    x = chain.prior((particles,), device=device)
    for _ in range(64):
        x = transition(x)

    def likelihood(yi, xi):
        return torch.softmax(torch.distributions.Normal(yi, sigma).log_prob(A(xi)).sum(dim=-1), 0)

    return metrics.bpf(x, y, transition, likelihood, step)[:, step:]


def timed(fn, warmup=2, runs=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/chain_posterior_bench.json')
    ap.add_argument('--particles', type=int, default=16384)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    chain = lorenz.make_chain()
    A = lambda x: chains.Lorenz63.preprocess(x)[..., :1]      # noqa: E731
    result = {'particles': args.particles, 'device': torch.cuda.get_device_name(0), 'warmup': 2, 'runs': 5, 'settings': {}}
    for name, s in SETTINGS.items():
        torch.manual_seed(0)
        x = chain.trajectory(chain.trajectory(chain.prior((), device=dev), 64, last=True), (s['nobs'] - 1) * s['step'] + 1)
        y = torch.normal(A(x[::s['step']]), s['sigma'])
        kw = dict(A=A, sigma=s['sigma'], step=s['step'], particles=args.particles)
        fused = timed(lambda: lorenz.posterior(y, fused=True, **kw))
        assert lorenz.LAST_POSTERIOR_ROUTE == 'fused'
        plain = timed(lambda: torch_route(y, device=dev, **kw))
        result['settings'][name] = {
            **s, 'transitions': 64 + s['nobs'] * s['step'],
            'fused_ms': [round(t * 1e3, 3) for t in fused], 'fused_median_ms': round(statistics.median(fused) * 1e3, 3),
            'torch_ms': [round(t * 1e3, 3) for t in plain], 'torch_median_ms': round(statistics.median(plain) * 1e3, 3),
        }
        result['settings'][name]['speedup'] = round(result['settings'][name]['torch_median_ms'] /
                                                    result['settings'][name]['fused_median_ms'], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
