"""ms per training step (loss, backward, AdamW) on three routes, alternating block by block in ONE process:

  uncaptured   sda_amd.training.AdamW(net=sde), the loss drawing t and eps from torch's generator (today's fused route)
  keyed        the same step with a training.KeyedLossNoise (csrc/train_loss.hip), still launch by launch
  graph        training.GraphedStep: the keyed step replayed as one hipGraph

Configurations: the Lorenz local kernel (LOCAL_CONFIG: window 5, embedding 32, width 256, depth 5) at batch 64 and 4096 windows; the
Lorenz global net (64,) x (3,) at batch 64 of (32, 3) and 1024 of (65, 3) with net1d=True; the Kolmogorov training net of
tools/train_bench.py at batch 32 with wgrad='tiled_ht' (10 steps per block).  Per route: the median of --blocks blocks of --steps steps
(wall clock around a synchronised block), the fastest and the slowest block.  The yardstick of a configuration is its uncaptured route
measured in the same run; ``faster`` is true only where the replayed median lies below the uncaptured route's FASTEST block.

    python tools/train_graph_bench.py --out profiles/train_graph_bench.json"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sda_amd import training  # noqa: E402
from sda_amd.score import VPSDE  # noqa: E402


def configs(dev, only):
    from sda_amd.experiments.kolmogorov import make_score
    from sda_amd.experiments.lorenz import make_global_score, make_local_score
    torch.manual_seed(0)
    out = []
    for batch in (64, 4096):
        out.append(dict(name=f'lorenz_local_b{batch}', make=lambda: make_local_score().kernel, shape=(15,), batch=batch, route=dict(mlp=True), steps=None))
    for batch, shape in ((64, (32, 3)), (1024, (65, 3))):
        out.append(dict(name=f'lorenz_global_b{batch}', make=lambda: make_global_score(embedding=32, hidden_channels=(64,), hidden_blocks=(3,)),
                        shape=shape, batch=batch, route=dict(mlp=True, net1d=True), steps=None))
    out.append(dict(name='kolmogorov_b32', steps=10, shape=(10, 64, 64), batch=32, route=dict(mlp=True, wgrad='tiled_ht'),
                    make=lambda: make_score(window=5, embedding=64, hidden_channels=(96, 192, 384), hidden_blocks=(3, 3, 3), size=64).kernel))
    return [c for c in out if not only or c['name'] in only]


def routes(cfg, dev):
    """{route: step function} on three copies of one net."""
    base = cfg['make']().to(dev)
    x = torch.randn(cfg['batch'], *cfg['shape'], device=dev)
    fns = {}
    for name in ('uncaptured', 'keyed', 'graph'):
        sde = VPSDE(copy.deepcopy(base), shape=cfg['shape']).to(dev)
        opt = training.AdamW(sde.parameters(), lr=1e-4, weight_decay=1e-3, net=sde)
        if name == 'graph':
            stepper = training.GraphedStep(sde, opt, seed=0, **cfg['route'])
            fns[name] = lambda stepper=stepper: stepper.step(x)
            continue
        noise = training.KeyedLossNoise(0) if name == 'keyed' else None
        sde.loss_noise = noise

        def step(sde=sde, opt=opt, noise=noise):
            with training.parameter_gradients(**cfg['route']):
                loss = sde.loss(x)
                loss.backward()
            opt.step()
            opt.zero_grad()
            if noise is not None:
                noise.counter().add_(1)
        fns[name] = step
    return fns


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, blocks=args.blocks, configs=[])
    for cfg in configs(dev, args.only):
        steps = cfg['steps'] or args.steps
        fns = routes(cfg, dev)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        ms = {name: [] for name in fns}
        for _ in range(args.blocks):
            for name, fn in fns.items():
                ms[name].append(block_ms(fn, steps))
        row = dict(name=cfg['name'], batch=cfg['batch'], shape=list(cfg['shape']), route=cfg['route'], steps_per_block=steps)
        for name, v in ms.items():
            row[name] = dict(median_ms=round(statistics.median(v), 4), fastest_ms=round(min(v), 4), slowest_ms=round(max(v), 4))
        row['faster'] = row['graph']['median_ms'] < row['uncaptured']['fastest_ms']
        row['graph_over_uncaptured'] = round(row['graph']['median_ms'] / row['uncaptured']['median_ms'], 4)
        result['configs'].append(row)
        print(json.dumps(row), flush=True)
        del fns
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
