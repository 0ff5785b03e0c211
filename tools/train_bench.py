"""Training-step benchmark of the opt-in parameter-gradient route (sda_amd.training).  bench.py (sampling) is not involved.

    python tools/train_bench.py [--steps 10] [--warmup 3] [--wgrad general|tiled|tiled_ht|both|all] [--blocks 5] [--out profiles/train_bench.json]

Reports, per configuration (Kolmogorov training net: LocalScoreUNet (96, 192, 384) x (3, 3, 3), embedding 64, batch 32 of
10 + 1 x 64 x 64; Lorenz global net: 1-D (64,) x (3,), batch 64 x 3 x 32):
  * ms per training step: VPSDE.loss + backward + AdamW.step on this package's kernels;
  * the same step with the oracle's functional net in fp32 under torch autograd on the same GPU (the stated baseline);
  * per-family kernel time of one step (ops.ConvProfile): forward convolutions, input-VJP convolutions, weight gradients,
    LayerNorm / modulation reductions, and the share of the torch-autograd modulation / time-embedding GEMMs;
and, for the Kolmogorov block shapes (96 ch @ 64^2, 192 @ 32^2, 384 @ 16^2, batch 32) and its four head and tail shapes (stride-2
heads 96 -> 192 @ 64^2 and 192 -> 384 @ 32^2, up-sampling tails 384 -> 192 @ 16^2 and 192 -> 96 @ 32^2), the weight-gradient kernel's
TFLOP/s and its fraction of the fp32 matrix peak (256 CUs x 4 SIMDs x 256 flop/clk x 2.4 GHz = 157.3 TFLOP/s).

--wgrad selects the weight-gradient route of the block convolutions (sda_amd.training: 'general' = csrc/conv_wgrad.hip everywhere,
'tiled' = csrc/conv_wgrad3.hip where it serves the launch, 'tiled_ht' = that and its stride-2 / up-sampling geometries for the heads and tails).
--wgrad both times the block shapes and the Kolmogorov step (and the
oracle's eager step) for the two routes ALTERNATING in one process, block by block (the scheme of tools/mlp_train_bench.py): per
block warm-up steps, then `steps` steps between two events; reported are the median of `blocks` blocks and the fastest and slowest
block.  The tiled route earns its place on a shape only where its median is below the general route's FASTEST block.  --wgrad all
does the same for general, tiled and tiled_ht (and the eager step), the head and tail shapes included: there tiled_ht is held to the
general route's fastest block per shape, and its step to the tiled route's fastest block.

--net1d times the Lorenz global net (lorenz_global_train) on the per-layer route (`layers`: what every training step of that net took
before training.enable(net1d=True) existed), on the whole-net kernels (`net1d`, csrc/net1d_train.hip) and on the oracle's eager step,
alternating block by block in one process, at batch 64 of (32, 3) and batch 1024 of (65, 3), each without and with the AdamW step (with
it the re-pack of the whole-net packings is in the number), plus the per-family launch counts and kernel times of one profiled `net1d`
step.  The `net1d` route earns its place where its median is below the `layers` route's FASTEST block."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import sda_oracle as O  # noqa: E402
from sda_amd import ops, training  # noqa: E402
from sda_amd.score import VPSDE  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
WGRAD_FAMILIES = ('wgrad', 'wgrad3', 'wgrad3x')


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def configs(dev):
    from sda_amd.experiments.kolmogorov import make_score
    from sda_amd.experiments.lorenz import make_global_score
    torch.manual_seed(0)
    kol = make_score(window=5, embedding=64, hidden_channels=(96, 192, 384), hidden_blocks=(3, 3, 3), size=64).kernel.to(dev)
    kol_cfg = O.UNetConfig(11, 10, 64, (96, 192, 384), (3, 3, 3), 3, 2, 'SiLU', 2, 'circular')
    lor = make_global_score(embedding=32, hidden_channels=(64,), hidden_blocks=(3,)).to(dev)
    lor_cfg = O.UNetConfig(3, 3, 32, (64,), (3,), 3, 2, 'SiLU', 1, 'zeros')
    return [
        dict(name='kolmogorov_train', net=kol, shape=(10, 64, 64), batch=32, prefix='',
             eps=lambda sd, x, t: O.score_unet(sd, '', kol_cfg, x, t, sd['forcing'])),
        dict(name='lorenz_global_train', net=lor, shape=(32, 3), batch=64, prefix='score.',
             eps=lambda sd, x, t: O.mc_score_wrapper(lambda xx, tt, c=None: O.score_unet(sd, 'score.', lor_cfg, xx, tt), x, t)),
    ]


def hip_step(cfg, dev, wgrad='general', net1d=False, optimizer=True):
    net = cfg['net']
    sde = VPSDE(net, shape=cfg['shape']).to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-3)
    x = torch.randn(cfg['batch'], *cfg['shape'], device=dev)

    def step():
        with training.parameter_gradients(wgrad=wgrad, net1d=net1d):
            loss = sde.loss(x)
            loss.backward()
        if optimizer:
            opt.step()
        opt.zero_grad()
    return step, sde, x


def oracle_step(cfg, dev, optimizer=True):
    """The same step on the oracle's functional net (fp32, torch autograd, the framework's own GPU kernels)."""
    names = {k for k, _ in cfg['net'].named_parameters()}
    sd = {k: v.detach().clone().float().to(dev).requires_grad_(k in names) for k, v in cfg['net'].state_dict().items()}
    opt = torch.optim.AdamW([sd[k] for k in sorted(names)], lr=1e-4, weight_decay=1e-3)
    sched = O.Schedule()
    x = torch.randn(cfg['batch'], *cfg['shape'], device=dev)

    def step():
        with torch.device(dev):                          # (the oracle builds its time-feature frequencies on the default device)
            t = torch.rand(x.shape[0], device=dev)
            e = torch.randn_like(x)
            tb = t.reshape((-1,) + (1,) * (x.dim() - 1))
            xt = sched.mu(tb) * x + sched.sigma(tb) * e
            loss = (cfg['eps'](sd, xt, t) - e).square().mean()
            loss.backward()
        if optimizer:
            opt.step()
        opt.zero_grad()
    return step


def family_profile(sde, x, wgrad='general', net1d=False):
    """One training step under ops.ConvProfile: kernel time by family, forward and backward apart."""
    prof = ops.ConvProfile()
    ops.conv_profile = prof
    try:
        with training.parameter_gradients(wgrad=wgrad, net1d=net1d):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            loss = sde.loss(x)
            e1.record()
            fwd_n = len(prof.records)
            fwd_mem = len(prof.mem_records)
            loss.backward()
            e2.record()
        torch.cuda.synchronize()
    finally:
        ops.conv_profile = None
    fam = {}
    for i, (a, b, flops, f) in enumerate(prof.records):
        key = f if f in WGRAD_FAMILIES + ('net1d_wgrad',) else ('forward.' if i < fwd_n else 'input_vjp.') + f
        r = fam.setdefault(key, dict(launches=0, ms=0.0, tflop=0.0))
        r['launches'] += 1
        r['ms'] += a.elapsed_time(b)
        r['tflop'] += flops / 1e12
    for i, (a, b, nb, k) in enumerate(prof.mem_records):
        key = ('forward.' if i < fwd_mem else 'backward.') + k
        r = fam.setdefault(key, dict(launches=0, ms=0.0, gbytes=0.0))
        r['launches'] += 1
        r['ms'] += a.elapsed_time(b)
        r['gbytes'] += nb / 1e9
    for r in fam.values():
        r['ms'] = round(r['ms'], 4)
        if 'tflop' in r:
            r['tflop_s'] = round(r['tflop'] / max(r['ms'], 1e-9) * 1e3, 2)
    for wg in (fam.get(f) for f in WGRAD_FAMILIES):
        if wg:
            wg['fraction_of_fp32_peak'] = round(wg['tflop_s'] * 1e12 / PEAK_FP32_MATRIX, 3)
    return dict(families=fam, loss_ms=round(e0.elapsed_time(e1), 3), backward_ms=round(e1.elapsed_time(e2), 3))


def modulation_share(cfg, dev, steps):
    """Time of the torch-autograd pieces of the route (time embedding + concatenated project Linear, forward and backward)."""
    net = cfg['net']
    kernel = net.score if cfg['prefix'] == 'score.' else net
    engine = kernel.network.engine()
    t = torch.rand(cfg['batch'], device=dev)

    def run():
        with training.parameter_gradients():
            emb = kernel.embedding(t)
            m = engine.modulation_train(emb)
            m.sum().backward()
    return _timed(run, steps, 2)


def _blocks(fns, steps, warmup, blocks):
    """{route: [ms per step of each block]}: the routes alternate block by block in this one process."""
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            out[k].append(_timed(fn, steps, warmup))
    return out


def _stat(ms):
    return dict(median_ms=round(statistics.median(ms), 4), fastest_ms=round(min(ms), 4), slowest_ms=round(max(ms), 4),
                blocks_ms=[round(v, 4) for v in ms])


def _block_layer(dev, c, s, n):
    """A block conv1 (modulation + LayerNorm loader, circular) at c channels, s x s."""
    from sda_amd.ops import make_conv_desc
    a = torch.randn(n, c, s, s, device=dev)
    mod = torch.randn(n, c, device=dev)
    mean = torch.zeros(n * s * s, device=dev)
    rstd = torch.ones(n * s * s, device=dev)
    g = torch.randn(n, c, s, s, device=dev)
    dw = torch.empty(c, c, 3, 3, device=dev)
    db = torch.empty(c, device=dev)
    d = make_conv_desc(x_ptr=a.data_ptr(), n=n, cx=c, hs=s, ws=s, x_sc=s * s, x_sy=s, x_sx=1, x_sn_outer=c * s * s, w_ptr=0,
                       cin_pad=0, cout_pad=0, cout=c, kh=3, kw=3, out_ptr=0, ho=s, wo=s, mt=1, circular=True,
                       mod_ptr=mod.data_ptr(), mod_sn=c, ln_mean_ptr=mean.data_ptr(), ln_rstd_ptr=rstd.data_ptr())
    return dict(channels=c, size=s, batch=n), d, g, dw, db, (a, mod, mean, rstd)


def _head_tail_layer(dev, kind, cin, cout, s, n):
    """A stride-2 head (plain loader) or an up-sampling tail (LayerNorm loader) reading cin channels at s x s, circular."""
    from sda_amd.ops import make_conv_desc
    so = s // 2 if kind == 'head_s2' else 2 * s
    a = torch.randn(n, cin, s, s, device=dev)
    mean = torch.zeros(n * s * s, device=dev)
    rstd = torch.ones(n * s * s, device=dev)
    g = torch.randn(n, cout, so, so, device=dev)
    dw = torch.empty(cout, cin, 3, 3, device=dev)
    db = torch.empty(cout, device=dev)
    extra = dict(stride_h=2, stride_w=2) if kind == 'head_s2' else dict(up_h=2, up_w=2, ln_mean_ptr=mean.data_ptr(),
                                                                         ln_rstd_ptr=rstd.data_ptr())
    d = make_conv_desc(x_ptr=a.data_ptr(), n=n, cx=cin, hs=s, ws=s, x_sc=s * s, x_sy=s, x_sx=1, x_sn_outer=cin * s * s, w_ptr=0,
                       cin_pad=0, cout_pad=0, cout=cout, kh=3, kw=3, out_ptr=0, ho=so, wo=so, mt=1, circular=True, **extra)
    return dict(layer=kind, cin=cin, cout=cout, size=s, out_size=so, batch=n), d, g, dw, db, (a, mean, rstd)


BLOCK_SHAPES = ((96, 64), (192, 32), (384, 16))
HEAD_TAIL_SHAPES = (('head_s2', 96, 192, 64), ('head_s2', 192, 384, 32), ('tail_up', 384, 192, 16), ('tail_up', 192, 96, 32))


def wgrad_shapes(dev, steps, routes=('general',), blocks=1, heads_tails=True):
    """The weight gradient at the three Kolmogorov block shapes (conv1: modulation + LayerNorm loader, circular) and, with
    ``heads_tails``, at its four head and tail shapes, batch 32.  With several routes: alternating blocks, and per shape whether the
    median of the route that serves it ('tiled' for the blocks, 'tiled_ht' for heads and tails) is below the general route's fastest
    block."""
    layers = [_block_layer(dev, c, s, 32) + ('tiled',) for c, s in BLOCK_SHAPES]
    if heads_tails:
        layers += [_head_tail_layer(dev, *spec, 32) + ('tiled_ht',) for spec in HEAD_TAIL_SHAPES]
    rows = []
    for head, d, g, dw, db, _keep, served_by in layers:
        flops = ops.wgrad_flops(d)
        if len(routes) == 1:
            ms = _timed(lambda: ops.conv_wgrad(d, g, dw, db, False, route=routes[0]), steps, 3)
            rows.append(dict(head, route=routes[0], ms=round(ms, 4), tflop_s=round(flops / ms / 1e9, 2),
                             fraction_of_fp32_peak=round(flops / ms / 1e9 * 1e12 / PEAK_FP32_MATRIX, 3)))
            continue
        times = _blocks({r: (lambda r=r: ops.conv_wgrad(d, g, dw, db, False, route=r)) for r in routes}, steps, 3, blocks)
        row = dict(head)
        for r in routes:
            st = _stat(times[r])
            st['tflop_s'] = round(flops / st['median_ms'] / 1e9, 2)
            st['fraction_of_fp32_peak'] = round(flops / st['median_ms'] / 1e9 * 1e12 / PEAK_FP32_MATRIX, 3)
            row[r] = st
        if served_by in routes:
            row[f'general_median_over_{served_by}_median'] = round(row['general']['median_ms'] / row[served_by]['median_ms'], 3)
            row[f'{served_by}_median_below_general_fastest'] = row[served_by]['median_ms'] < row['general']['fastest_ms']
        rows.append(row)
    return rows


def kolmogorov_routes(cfg, dev, steps, warmup, blocks, routes=('general', 'tiled')):
    """The Kolmogorov training step on the weight-gradient routes and the oracle's eager step, alternating block by block."""
    fns = {r: hip_step(cfg, dev, r)[0] for r in routes}
    fns['eager'] = oracle_step(cfg, dev)
    times = _blocks(fns, steps, warmup, blocks)
    out = {k: _stat(v) for k, v in times.items()}
    for r in routes:
        out[f'{r}_over_eager'] = round(out['eager']['median_ms'] / out[r]['median_ms'], 3)
    out['tiled_step_below_eager'] = out['tiled']['median_ms'] < out['eager']['median_ms']
    if 'tiled_ht' in routes:
        out['tiled_ht_median_below_tiled_fastest'] = out['tiled_ht']['median_ms'] < out['tiled']['fastest_ms']
    return out


NET1D_CONFIGS = ((64, (32, 3)), (1024, (65, 3)))


def net1d_routes(dev, steps, warmup, blocks):
    """The Lorenz global net's training step on the per-layer route, the whole-net route and the oracle's eager step."""
    base = [c for c in configs(dev) if c['name'] == 'lorenz_global_train'][0]
    rows = []
    for batch, shape in NET1D_CONFIGS:
        cfg = dict(base, batch=batch, shape=shape)
        row = dict(batch=batch, shape=list(shape))
        for optimizer in (False, True):
            fns = dict(layers=hip_step(cfg, dev, optimizer=optimizer)[0], net1d=hip_step(cfg, dev, net1d=True, optimizer=optimizer)[0],
                       eager=oracle_step(cfg, dev, optimizer=optimizer))
            out = {k: _stat(v) for k, v in _blocks(fns, steps, warmup, blocks).items()}
            out['layers_median_over_net1d_median'] = round(out['layers']['median_ms'] / out['net1d']['median_ms'], 3)
            out['eager_median_over_net1d_median'] = round(out['eager']['median_ms'] / out['net1d']['median_ms'], 3)
            out['net1d_median_below_layers_fastest'] = out['net1d']['median_ms'] < out['layers']['fastest_ms']
            row['with_adamw_step' if optimizer else 'loss_and_backward'] = out
        step, sde, x = hip_step(cfg, dev, net1d=True)
        step()
        row['net1d_profile'] = family_profile(sde, x, net1d=True)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wgrad', choices=('general', 'tiled', 'tiled_ht', 'both', 'all'), default='general')
    ap.add_argument('--blocks', type=int, default=5, help='--wgrad both / all: blocks per route (median, fastest and slowest are reported)')
    ap.add_argument('--net1d', action='store_true', help='the Lorenz global net: per-layer route, whole-net route and eager, alternating')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.net1d:
        result = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, warmup=args.warmup, blocks=args.blocks,
                      lorenz_global_train=net1d_routes(dev, args.steps, args.warmup, args.blocks), time=time.strftime('%Y-%m-%dT%H:%M:%S'))
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(result, f, indent=1)
        return
    route = {'both': 'tiled', 'all': 'tiled_ht'}.get(args.wgrad, args.wgrad)
    compared = {'both': ('general', 'tiled'), 'all': ('general', 'tiled', 'tiled_ht')}.get(args.wgrad)
    result = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, warmup=args.warmup, wgrad=args.wgrad, configs={})
    if compared:
        result['blocks'] = args.blocks
        result['wgrad_block_shapes'] = wgrad_shapes(dev, args.steps, compared, args.blocks, heads_tails='tiled_ht' in compared)
        print(json.dumps({'wgrad_block_shapes': result['wgrad_block_shapes']}), flush=True)
    for cfg in configs(dev):
        if compared and cfg['name'] != 'kolmogorov_train':
            continue                                     # (1-D nets keep the general kernel under either setting)
        step, sde, x = hip_step(cfg, dev, route)
        ms = _timed(step, args.steps, args.warmup)
        prof = family_profile(sde, x, route)
        mod_ms = modulation_share(cfg, dev, args.steps)
        base_ms = _timed(oracle_step(cfg, dev), args.steps, args.warmup)
        result['configs'][cfg['name']] = dict(
            batch=cfg['batch'], shape=list(cfg['shape']), ms_per_step=round(ms, 3), oracle_fp32_autograd_ms_per_step=round(base_ms, 3),
            speedup_vs_oracle=round(base_ms / ms, 3), modulation_autograd_ms=round(mod_ms, 4),
            modulation_share_of_step=round(mod_ms / ms, 4), profile=prof)
        if compared:
            result['configs'][cfg['name']]['profiled_route'] = route
            result['configs'][cfg['name']]['routes'] = kolmogorov_routes(cfg, dev, args.steps, args.warmup, args.blocks, compared)
        print(json.dumps({cfg['name']: result['configs'][cfg['name']]}), flush=True)
    if not compared:
        result['wgrad_block_shapes'] = wgrad_shapes(dev, args.steps, (args.wgrad,))
    result['time'] = time.strftime('%Y-%m-%dT%H:%M:%S')
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
