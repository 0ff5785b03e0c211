#!/usr/bin/env python3
"""Wall-clock of the reference's evaluation protocol (experiments/lorenz/eval.py:72-84: six posterior-sampling runs of 1024 trajectories x
256 steps with C = 0, 1, 2, 4, 8, 16 corrections) for the LOCAL score net at a chosen width -- 256 is what the reference trains
(experiments/lorenz/train.py:30-44); bench.py's lorenz_eval runs make_local_score()'s default 128.  Same six runs as bench.run_lorenz_eval,
each replayed from a captured hipGraph; one JSON object on stdout (and in --json FILE).

    python tools/lorenz_eval_wide.py [--width 256] [--window 5] [--repeats 3] [--freq lo] [--json FILE]
    python tools/lorenz_eval_wide.py --window 7 ...             # eval.py's k = 3 checkpoint (k = 4: --window 9)
    SDA_MLP_FUSED=0 python tools/lorenz_eval_wide.py ...        # the per-layer route, the A/B partner
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--depth', type=int, default=5)
    ap.add_argument('--window', type=int, default=5, help='states per window, 2k + 1 (eval.py: 3, 5, 7, 9)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--freq', default='lo', choices=sorted(bench.LORENZ_EVAL_FREQ))
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    from sda_amd import fused1d, mlp, observe as Ob
    from sda_amd.experiments.lorenz import make_local_score
    from sda_amd.score import GaussianScore, VPSDE
    dev = torch.device('cuda:0')
    step, std = bench.LORENZ_EVAL_FREQ[args.freq]
    B, L, S, steps = args.batch, 65, 3, 256
    torch.manual_seed(0)
    net = make_local_score(window=args.window, width=args.width, depth=args.depth)
    score = bench.SyntheticScore(net)
    inner = VPSDE(score, shape=())
    object.__setattr__(score, '_sched', inner)
    y = torch.randn((L + step - 1) // step, 1, generator=torch.Generator().manual_seed(2))
    gs = GaussianScore(y, A=Ob.Subsample((slice(None, None, step), slice(0, 1))), std=std, sde=inner, gamma=3e-2)
    sde = VPSDE(gs, shape=(L, S)).to(dev)
    wu = sde.sampler((B,), steps=steps, corrections=1, tau=0.25)
    route = type(wu._fused).__name__ if wu._fused is not None else 'general'
    for _ in range(3):
        wu.step()
    torch.cuda.synchronize(dev)
    totals, finite = [], True
    for _rep in range(args.repeats):
        torch.manual_seed(1)
        loop_s = 0.0
        for C in (0, 1, 2, 4, 8, 16):
            sampler = sde.sampler((B,), steps=steps, corrections=C, tau=0.25)
            sampler.capture()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(steps):
                sampler.step()
            torch.cuda.synchronize(dev)
            loop_s += time.perf_counter() - t1
            finite = finite and bool(torch.isfinite(sampler.result()).all().item())
        totals.append(loop_s)
    out = {'workload': 'lorenz_eval protocol, local net', 'width': args.width, 'depth': args.depth, 'window': args.window, 'freq': args.freq, 'batch': B,
           'mlp_fused': mlp.FUSED, 'fused1d': fused1d.ENABLED, 'route': route, 'score_evals': steps * 37, 'six_run_sampling_s': totals,
           'min_s': min(totals), 'median_s': statistics.median(totals), 'max_s': max(totals),
           'ms_per_score_eval_median': statistics.median(totals) / (steps * 37) * 1e3, 'samples_finite': finite}
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f)


if __name__ == '__main__':
    main()
