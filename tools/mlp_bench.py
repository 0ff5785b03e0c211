#!/usr/bin/env python3
"""HIP-event timing of the whole-MLP kernels (csrc/mlp1d.hip) on the Lorenz local kernel at eval.py's batch (1024 x 61 windows).

    python tools/mlp_bench.py [rows] [--width 128] [--depth 5] [--json FILE]

--width 256 is the reference's trained local net (the _wide kernels); SDA_MLP_FUSED=0 times the per-layer route on the same net."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sda_amd.nn import ResMLP
from sda_amd.utils import ACTIVATIONS
dev = torch.device('cuda:0')
ap = argparse.ArgumentParser()
ap.add_argument('rows', nargs='?', type=int, default=1024 * 61)
ap.add_argument('--width', type=int, default=128)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--json', default=None, help='also write the figures to this file')
args = ap.parse_args()
rows, W, D = args.rows, args.width, args.depth
net = ResMLP(47, 15, hidden_features=[W] * D, activation=ACTIVATIONS['SiLU']).to(dev)
res = {'rows': rows, 'width': W, 'depth': D, 'fused': os.environ.get('SDA_MLP_FUSED', '1') != '0'}
x = torch.randn(rows, 47, device=dev, requires_grad=True)
g = torch.randn(rows, 15, device=dev)
flops = 2.0 * rows * (47 * W + 2 * D * W * W + W * 15 + 2 * 15 * 15)
for name, fn in (('(clock ramp: discard)', lambda: net(x)), ('fwd (no saves)', lambda: net(x.detach())), ('fwd + saves', lambda: net(x)),):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20): fn()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    print(f'{name:16s} {ms * 1e3:8.1f} us   {flops / ms / 1e9:7.1f} TFLOP/s ({flops / ms / 1e9 / 157.3:.3f} of the fp32 MFMA peak)')
    res[name] = {'us': ms * 1e3, 'peak_fraction': flops / ms / 1e9 / 157.3}
out = net(x)
for _ in range(10): torch.autograd.grad(out, x, g, retain_graph=True)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): torch.autograd.grad(out, x, g, retain_graph=True)
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 20
print(f'{"VJP":16s} {ms * 1e3:8.1f} us   {flops / ms / 1e9:7.1f} TFLOP/s ({flops / ms / 1e9 / 157.3:.3f})')
res['VJP'] = {'us': ms * 1e3, 'peak_fraction': flops / ms / 1e9 / 157.3}
res.pop('(clock ramp: discard)', None)
if args.json:
    with open(args.json, 'w') as f:
        json.dump(res, f)
