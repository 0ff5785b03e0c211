#!/usr/bin/env python3
"""Randomised parity sweep of the training route (sda_amd.training): every parameter gradient and the input gradient of whole
score networks, formed in ONE backward, against torch.autograd through the oracle evaluated in float64.

    python tests/fuzz/train_fuzz.py [--cases 60] [--seed 0] [--chunk K]

The architectures and shapes are those of net_fuzz.py (1-3 levels, 1-3 blocks, widths incl. the multiples of 32 / 96 whose
forward takes the Winograd kernels while the weight gradient reads the same saved activations, 1-D / 2-D, zero / circular
padding, MC windows, context, shared or per-sample times).  ``--chunk K`` forces the engine through recomputed chunks of K
images.  With ``dev = cpu`` the case runs on the host replay (tests/cpu_shim.py must be installed by the caller)."""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import sda_oracle as O  # noqa: E402
from sda_amd import engine as E  # noqa: E402
from sda_amd import training  # noqa: E402
from sda_amd.score import MCScoreNet, ScoreUNet  # noqa: E402

ACTS = {'SiLU': nn.SiLU, 'GELU': nn.GELU, 'ELU': nn.ELU, 'ReLU': nn.ReLU, 'SELU': nn.SELU}
SMOOTH = ('SiLU', 'GELU', 'ELU')                 # no kink: no case of these is ever skipped
TOL = 1e-4


def _min_preact(run):
    """min |z| over every activation input of one oracle evaluation (as net_fuzz.py)."""
    seen, orig = [], O.activation

    def recording(name):
        f = orig(name)

        def g(z):
            seen.append(z.detach().abs().min().item())
            return f(z)
        return g
    O.activation = recording
    try:
        with torch.no_grad():
            run()
    finally:
        O.activation = orig
    return min(seen) if seen else 1.0


class forced_chunks:
    """Within the block the engine keeps nothing and recomputes its forward inside the backward, ``chunk`` images at a time."""

    def __init__(self, chunk):
        self.chunk = chunk

    def __enter__(self):
        self.orig = E.UNetEngine.chunk_size
        if self.chunk is not None:
            k = self.chunk
            E.UNetEngine.chunk_size = lambda self, n, hs, ws, save, device, fraction=None: min(n, k)

    def __exit__(self, *exc):
        E.UNetEngine.chunk_size = self.orig


def one_case(rng, dev, idx, chunk=None, acts=tuple(ACTS), small=False):
    """small: narrow nets and small images only (the host replay runs every multiply in scalar code)."""
    dev = torch.device(dev)
    spatial = rng.choice([1, 2, 2])
    depth = rng.choice([1, 2, 2, 3])
    widths = {1: [4, 8, 24, 32, 64, 96], 2: [4, 8, 16, 32, 64, 96], 3: [4, 8, 32]}[depth]
    if small:
        widths = [3, 4, 8]
    c0 = rng.choice(widths)
    hidden = tuple(c0 * 2 ** i for i in range(depth))
    blocks = tuple(rng.choice([1, 2] if small else [1, 2, 3]) for _ in range(depth))
    act = rng.choice(list(acts))
    pad = rng.choice(['zeros', 'circular'])
    mc = rng.random() < 0.5
    state = rng.choice([1, 2, 3])
    order = rng.choice([1, 2]) if mc else 0
    channels = state * (2 * order + 1) if mc else rng.choice([1, 2, 3, 5])
    context = rng.choice([0, 0, 1, 2]) if not mc else 0
    mult = 2 ** (depth - 1)
    size = [mult * rng.choice([1, 2, 3, 4] if small else [1, 2, 3, 4, 8]) for _ in range(spatial)]
    if spatial == 2 and c0 >= 64:
        size = [min(s, 16) for s in size]
    emb = rng.choice([8, 16])
    cfg = dict(idx=idx, spatial=spatial, hidden=hidden, blocks=blocks, act=act, pad=pad, mc=mc, order=order, channels=channels,
               context=context, size=size, chunk=chunk)
    torch.manual_seed(9000 + idx)
    kw = dict(embedding=emb, hidden_channels=hidden, hidden_blocks=blocks, kernel_size=3, activation=ACTS[act],
              spatial=spatial, padding_mode=pad)
    ocfg = O.UNetConfig(channels + context, channels, emb, hidden, blocks, 3, 2, act, spatial, pad)
    B = rng.choice([1, 2, 3])
    per_sample_t = rng.random() < 0.5
    if mc:
        net = MCScoreNet(state, order=order, **kw)
        L = 2 * order + rng.choice([1, 2, 4])
        x = torch.randn(B, L, state, *size)
        t = torch.rand(B, L - 2 * order) if per_sample_t else torch.rand(())    # one time per window, or one for all
        c = None
    else:
        net = ScoreUNet(channels, context, **kw)
        x = torch.randn(B, channels, *size)
        t = torch.rand(B) if per_sample_t else torch.rand(())
        c = torch.randn(B, context, *size) if context else None
    cfg.update(B=B, per_sample_t=per_sample_t, x=tuple(x.shape))
    for p in net.parameters():                       # widen the default init so that every path carries signal
        p.data.mul_(1.5)
    names = [k for k, _ in net.named_parameters()]
    sd = {k: v.detach().double().clone().requires_grad_(k in names) for k, v in net.state_dict().items()}

    def oracle(xx, tt, cc):
        if mc:
            kern = lambda a, b, _c=None: O.score_unet(sd, 'kernel.', ocfg, a, b, None)
            return O.mc_score_net(kern, order, xx, tt)
        return O.score_unet(sd, '', ocfg, xx, tt, cc)

    c64 = None if c is None else c.double()
    if act in ('ReLU', 'SELU') and _min_preact(lambda: oracle(x.double(), t.double(), c64)) < 2e-5:
        return cfg, 'SKIP'                           # (the kink rule of net_fuzz.py: act'(z) flips within fp32 round-off of 0)
    xo = x.double().requires_grad_(True)
    ref = oracle(xo, t.double(), c64)
    g = torch.randn(ref.shape, dtype=torch.float64)
    want = torch.autograd.grad(ref, [xo] + [sd[k] for k in names], g, allow_unused=True)
    net = net.to(dev)
    xs = x.to(dev).requires_grad_(True)
    try:
        with forced_chunks(chunk), training.parameter_gradients():
            out = net(xs, t.to(dev)) if c is None else net(xs, t.to(dev), c.to(dev))
            out.backward(g.float().to(dev))
    except Exception as e:  # noqa: BLE001
        return cfg, f'EXCEPTION {type(e).__name__}: {e}'
    got = [out.detach(), xs.grad] + [p.grad for _, p in net.named_parameters()]
    for name, a, b in zip(['forward', 'x'] + names, got, [ref.detach()] + list(want)):
        if b is None:                                # (a parameter the output does not depend on)
            if a is not None and a.abs().max().item() != 0:
                return cfg, f'{name}: a gradient where the oracle has none'
            continue
        if a is None:
            return cfg, f'{name}: no gradient formed'
        a = a.detach().cpu().double()
        if not torch.isfinite(a).all():
            return cfg, f'{name}: non-finite'
        scale = b.abs().max().item() + 1e-30
        err = (a - b).abs().max().item()
        if err > TOL * scale:
            return cfg, f'{name}: max abs err {err:.3e} vs scale {scale:.3e}'
    return cfg, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=60)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk', type=int, default=0, help='force recomputed chunks of this many images on every second case')
    args = ap.parse_args()
    rng = random.Random(args.seed)
    dev = torch.device('cuda:0')
    bad = skipped = 0
    for i in range(args.cases):
        cfg, msg = one_case(rng, dev, i + 7919 * args.seed, chunk=args.chunk if (args.chunk and i % 2) else None)
        if msg == 'SKIP':
            skipped += 1
            continue
        if msg:
            bad += 1
            print(f'FAIL case {i}: {msg}\n     {cfg}', flush=True)
    print(f'{args.cases - bad - skipped}/{args.cases - skipped} networks within {TOL:g} (forward, input gradient and every parameter '
          f'gradient); {skipped} ill-conditioned cases skipped (a ReLU/SELU pre-activation within 2e-5 of its kink)')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
