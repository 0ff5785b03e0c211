#!/usr/bin/env python3
"""The two variational baselines of the Lorenz experiment on their two gradient routes, alternating in one process: ``grad='device'``
(the chain kernels of csrc/chain.hip and their adjoint) and ``grad='torch'`` (torch autograd through the torch-ops rk4).

    python tools/lorenz_4dvar_bench.py [--out profiles/lorenz_4dvar_bench.json]

weak:   ``lorenz.weak_4d_var`` on a 65 x 3 trajectory of ``make_chain()``, step = 8, the reference's observation
        A(x) = preprocess(x)[..., :1] with sigma = 0.05, 16 L-BFGS iterations -- what the reference's figures run per posterior sample.
strong: ``lorenz.strong_4d_var`` over the initial state of ``Lorenz63(dt=0.025)`` for the first 32 of those transitions, same A, sigma, step.

A block is one whole optimisation on each route, torch first; the figure is the median over 5 blocks after one warm-up of each route,
torch.cuda.synchronize() around every call, with the fastest and the slowest block recorded.  The kernels are latency-bound by design:
what is compared is the number of launches per closure call, not arithmetic throughput.  The objective each route ends at is
recorded too; the iterates themselves are not compared (L-BFGS amplifies rounding differences).
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

A = lambda x: chains.Lorenz63.preprocess(x)[..., :1]  # noqa: E731  (experiments/lorenz/eval.py of the reference)
SIGMA, STEP, LENGTH, STRONG = 0.05, 8, 65, 32


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(args):
    torch.manual_seed(args.seed)
    dev = torch.device(args.device)
    chain = lorenz.make_chain()
    with torch.no_grad():
        x0 = chain.trajectory(chain.prior((1,), device=dev), length=64, last=True, seed=args.seed)      # burn-in, as posterior() does
        truth = torch.cat((x0, chain.trajectory(x0, LENGTH - 1, seed=args.seed + 1)[:, 0]))              # (65, 3)
        y = A(truth[::STEP]) + SIGMA * torch.randn(len(truth[::STEP]), 1, device=dev)
        x_init = truth + 0.5 * torch.randn_like(truth)
        det = chains.Lorenz63(dt=0.025)
        y_strong = A(det.trajectory(x0, STRONG)[:, 0][::STEP])
        x_b = x0[0] + 0.1 * torch.randn(3, device=dev)

    def weak_objective(x):
        return float((x[0] - x_init[0]).square().sum() - lorenz.log_prior(x) - lorenz.log_likelihood(y, x, A, SIGMA, STEP))

    def strong_objective(x):
        return float((x - x_b).square().sum() + ((y_strong - A(det.trajectory(x, STRONG)[::STEP])).square() / SIGMA ** 2).sum())

    def weak(route):
        out = lorenz.weak_4d_var(x_init, y, A, SIGMA, STEP, iterations=args.iterations, grad=route)
        assert chains.LAST_CHAIN_GRAD_ROUTE == route
        return out

    def strong(route):
        out = lorenz.strong_4d_var(x_b, y_strong, A, SIGMA, STEP, iterations=args.iterations, chain=chains.Lorenz63(dt=0.025, grad=route))
        assert chains.LAST_CHAIN_GRAD_ROUTE == route
        return out

    result = {'length': LENGTH, 'strong_transitions': STRONG, 'step': STEP, 'sigma': SIGMA, 'iterations': args.iterations, 'blocks': args.blocks,
              'device': torch.cuda.get_device_name(0), 'cases': []}
    for name, run, objective, start in (('weak_4d_var', weak, weak_objective, x_init), ('strong_4d_var', strong, strong_objective, x_b)):
        with torch.no_grad():
            case = {'case': name, 'objective_at_start': objective(start)}
        finals = {r: run(r) for r in ('torch', 'device')}                 # warm-up of each route
        times = {'torch': [], 'device': []}
        for _ in range(args.blocks):
            for r in ('torch', 'device'):
                times[r].append(once(lambda: run(r))[0])
        for r in ('device', 'torch'):
            with torch.no_grad():
                case[f'{r}_objective_at_end'] = objective(finals[r])
            case.update({f'{r}_ms': [round(t * 1e3, 3) for t in times[r]], f'{r}_median_ms': round(statistics.median(times[r]) * 1e3, 3),
                         f'{r}_fastest_ms': round(min(times[r]) * 1e3, 3), f'{r}_slowest_ms': round(max(times[r]) * 1e3, 3)})
        case['device_median_below_fastest_torch_block'] = statistics.median(times['device']) < min(times['torch'])
        result['cases'].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--iterations', type=int, default=16)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--device', default='cuda')
    p.add_argument('--out', default='profiles/lorenz_4dvar_bench.json')
    main(p.parse_args())
