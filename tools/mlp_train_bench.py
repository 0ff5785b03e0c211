"""ms per training step (loss, backward, AdamW step) of the Lorenz LOCAL score kernel -- the reference's LOCAL_CONFIG: ScoreNet(15,
embedding 32) over a ResMLP 47 -> 256 x 5 -> 15, SiLU -- on the device route (sda_amd.training.parameter_gradients(mlp=True),
csrc/mlp_train.hip) against the same network as plain torch.nn modules under PyTorch eager autograd, on the same GPU in the same process,
and a third route, the device route with this project's optimizer (sda_amd.training.AdamW, csrc/optim.hip: one launch, the plan's weight slabs stay
packed) -- the three alternating block by block; per batch also loss + backward alone (no optimizer step) of each route.  Batch 64 is train_local's;
4096 is the row count of MCScoreNet training.

    python tools/mlp_train_bench.py [--iters 200] [--blocks 5] [--out profiles/mlp_train_bench.json]

Per block and route: warm-up steps, then `iters` steps between two events; the figure reported is the median block.  The launch count is
the number of this project's kernels one ResMLP forward + backward issues (the time embedding and the loss are torch's on every route, AdamW
on the first two); `fused_step_launches` adds the optimizer launches of the third route.  `fused_optimizer_ms` = the fused step minus
loss + backward alone."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _TorchBlock(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.l1, self.l2 = nn.Linear(w, w), nn.Linear(w, w)

    def forward(self, x):
        var, mean = torch.var_mean(x, dim=-1, keepdim=True)          # (one fused statistics op, unbiased variance: as the modelled LayerNorm)
        h = (x - mean) / (var + 1e-5).sqrt()
        return x + self.l2(torch.nn.functional.silu(self.l1(h)))


class _TorchScoreNet(nn.Module):
    """LOCAL_CONFIG as plain torch.nn: the yardstick."""

    def __init__(self, features=15, embedding=32, width=256, depth=5):
        super().__init__()
        self.emb = nn.Sequential(nn.Linear(32, 256), nn.SiLU(), nn.Linear(256, embedding))
        self.register_buffer('freqs', torch.pi * torch.arange(1, 17))
        self.net = nn.Sequential(nn.Linear(features + embedding, width), *[_TorchBlock(width) for _ in range(depth)],
                                 nn.Linear(width, features), _TorchBlock(features))

    def forward(self, x, t):
        ang = t.reshape(-1, 1) * self.freqs
        return self.net(torch.cat((x, self.emb(torch.cat((torch.cos(ang), torch.sin(ang)), dim=-1))), dim=-1))


def _torch_loss(net, x):
    t = torch.rand(x.shape[0], device=x.device)
    alpha = torch.cos(1.5391588111080307 * t) ** 2          # acos(sqrt(1e-3)): the 'cos' schedule of VPSDE
    mu, sigma = alpha.reshape(-1, 1), (1 - alpha ** 2 + 1e-6).sqrt().reshape(-1, 1)
    eps = torch.randn_like(x)
    return (net(mu * x + sigma * eps, t) - eps).square().mean()


def _time(step, warmup, iters):
    for _ in range(warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 4096])
    ap.add_argument('--out', default=os.path.join('profiles', 'mlp_train_bench.json'))
    args = ap.parse_args()
    from sda_amd import ops, training
    from sda_amd.experiments.lorenz import make_local_score
    from sda_amd.score import VPSDE
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    kernel = make_local_score(width=256, depth=5).kernel.to(dev)
    sde = VPSDE(kernel, shape=(15,)).to(dev)
    ref = _TorchScoreNet().to(dev)
    opt_hip = torch.optim.AdamW(kernel.parameters(), lr=1e-3, weight_decay=1e-3)
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-3)
    opt_fused = training.AdamW(kernel.parameters(), lr=1e-3, weight_decay=1e-3, net=kernel)

    # launches of this project's kernels per ResMLP forward + backward
    counts = {'n': 0}
    wrapped = {}
    for name, k in (('mlp_launch', 1), ('mlp_bwd_train', 1), ('mlp_wgrad', 2), ('adamw_step', 1)):
        fn = getattr(ops, name)
        wrapped[name] = fn
        setattr(ops, name, (lambda f, kk: lambda *a, **kw: (counts.__setitem__('n', counts['n'] + kk), f(*a, **kw))[1])(fn, k))
    with training.parameter_gradients(mlp=True):
        sde.loss(torch.randn(64, 15, device=dev)).backward()
    launches = counts['n']
    opt_fused.step()
    fused_launches = counts['n']
    for name, fn in wrapped.items():
        setattr(ops, name, fn)
    opt_fused.zero_grad()

    result = {'network': 'ScoreNet(15, embedding=32) / ResMLP 47 -> 256 x 5 -> 15 -> block(15), SiLU (LOCAL_CONFIG)',
              'step': 'VPSDE loss + backward + AdamW step', 'iters': args.iters, 'warmup': args.warmup, 'blocks': args.blocks,
              'resmlp_launches_per_step': launches, 'fused_step_launches': fused_launches, 'device': torch.cuda.get_device_name(0), 'batches': {}}
    try:
        result['clock_mhz'] = torch.cuda.clock_rate()
    except Exception as e:  # noqa: BLE001 -- the SMI binding is optional
        result['clock_mhz'] = f'unavailable ({type(e).__name__})'
    for batch in args.batches:
        x = torch.randn(batch, 15, device=dev)

        def step_hip():
            with training.parameter_gradients(mlp=True):
                sde.loss(x).backward()
            opt_hip.step()
            opt_hip.zero_grad()

        def step_fused():
            with training.parameter_gradients(mlp=True):
                sde.loss(x).backward()
            opt_fused.step()
            opt_fused.zero_grad()

        def step_ref():
            _torch_loss(ref, x).backward()
            opt_ref.step()
            opt_ref.zero_grad()
        hip, fused, eager = [], [], []
        for _ in range(args.blocks):                      # alternate the three routes
            hip.append(_time(step_hip, args.warmup, args.iters))
            fused.append(_time(step_fused, args.warmup, args.iters))
            eager.append(_time(step_ref, args.warmup, args.iters))
        h, fu, r = statistics.median(hip), statistics.median(fused), statistics.median(eager)

        # where the time goes: loss + backward alone (gradients accumulate; no optimizer step), one block per route
        def fb_hip():
            with training.parameter_gradients(mlp=True):
                sde.loss(x).backward()

        def fb_ref():
            _torch_loss(ref, x).backward()
        fh, fr = _time(fb_hip, args.warmup, args.iters), _time(fb_ref, args.warmup, args.iters)
        opt_hip.zero_grad()
        opt_ref.zero_grad()
        # the optimizer's cost on the fused route: one more block of the fused step right behind loss + backward alone
        ff = _time(step_fused, args.warmup, args.iters)
        result['batches'][str(batch)] = {'device_route_ms': h, 'torch_eager_ms': r, 'eager_over_device': r / h,
                                         'device_route_loss_backward_ms': fh, 'torch_eager_loss_backward_ms': fr,
                                         'device_route_blocks_ms': hip, 'torch_eager_blocks_ms': eager,
                                         'fused_route_ms': fu, 'eager_over_fused': r / fu, 'device_over_fused': h / fu,
                                         'fused_route_blocks_ms': fused,
                                         'fused_slowest_below_device_fastest': max(fused) < min(hip),
                                         'fused_route_step_after_loss_backward_ms': ff, 'fused_optimizer_ms': ff - fh}
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
