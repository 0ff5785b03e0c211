"""Shared helpers for the test-suite (fixtures are data only: tests/golden/*.npz)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    """Returns (arrays, groups): flat entries as tensors, 'group/key' entries nested by group."""
    data = np.load(os.path.join(GOLDEN, name + '.npz'))
    flat, groups = {}, {}
    for k in data.files:
        v = torch.from_numpy(np.asarray(data[k]))
        if '/' in k:
            g, kk = k.split('/', 1)
            groups.setdefault(g, {})[kk] = v
        else:
            flat[k] = v
    return flat, groups


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def assert_close(a, b, rtol=1e-4, atol=None, what=''):
    """max|a-b| <= rtol * max|b| (+atol): the scale-relative form of north_star's rtol=1e-4 (fp32)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, f'{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}'
    scale = b.abs().max().item()
    tol = rtol * scale + (atol or 0.0)
    diff = (a - b).abs()
    err = diff.max().item() if diff.numel() else 0.0
    assert err <= tol, f'{what}: max abs err {err:.3e} > {tol:.3e} (scale {scale:.3e})'
    # and elementwise: |a - b| <= rtol |b| + atol_e with atol_e = rtol/10 x the tensor scale (not below fp32 round-off of
    # that scale), i.e. torch.allclose(a, b, rtol, atol_e)
    atol_e = max(0.1 * rtol, 2e-6) * scale + (atol or 0.0)
    bound = rtol * b.abs() + atol_e
    bad = diff > bound
    if bad.any():
        worst = (diff - bound).argmax().item()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside rtol={rtol:g}, '
                             f'atol={atol_e:.3e}; worst |a-b|={diff.reshape(-1)[worst]:.3e} '
                             f'at |b|={b.abs().reshape(-1)[worst]:.3e}')


def load_conv_dispatch():
    """tests/golden/conv_dispatch.json, the direct-kernel dispatch recorded before conv_pick existed: the list of cases.
    A case is a dict of the descriptor's integer fields, the four switches, `direct` (no other kernel family takes the launch),
    `rc`, and on rc == 0 `pick` (kernel, mt, nt, spad, kh, kw, ck, npos) and `geom` (tn, tr, tw, S, grid, nstage, wide_out, lds bytes)."""
    import json
    with open(os.path.join(GOLDEN, 'conv_dispatch.json')) as f:
        data = json.load(f)
    nd, ns = len(data['desc_fields']), len(data['switch_fields'])
    cases = []
    for row in data['cases']:
        c = dict(zip(data['desc_fields'], row[:nd]))
        c['switches'] = tuple(row[nd:nd + ns])
        c['direct'], c['rc'] = row[nd + ns], row[nd + ns + 1]
        c['pick'], c['geom'] = tuple(row[nd + ns + 2:nd + ns + 10]), tuple(row[nd + ns + 10:])
        cases.append(c)
    return cases


def conv_dispatch_desc(c, x_ptr=0x10000, w_ptr=0x20000, out_ptr=0x30000, **ptrs):
    """The sda_conv_desc of a load_conv_dispatch() case: a planar source; `misalign` bytes are added to the output address."""
    from sda_amd.ops import make_conv_desc
    return make_conv_desc(x_ptr=x_ptr, n=c['n'], cx=c['cx'], hs=c['hs'], ws=c['ws'], x_sc=c['hs'] * c['ws'], x_sy=c['ws'], x_sx=1,
                          x_sn_outer=c['cx'] * c['hs'] * c['ws'], w_ptr=w_ptr, cin_pad=c['cin_pad'], cout_pad=c['cout_pad'],
                          cout=c['cout'], kh=c['kh'], kw=c['kw'], out_ptr=out_ptr + c['misalign'], ho=c['ho'], wo=c['wo'], mt=c['mt'],
                          stride_h=c['stride_h'], stride_w=c['stride_w'], circular=c['circular'],
                          pad=(c['pad_h'], c['pad_w']) if c['explicit_pad'] else None, **ptrs)


def load_pick_dispatch(name):
    """tests/golden/wino4_dispatch.json / h2_dispatch.json, the dispatch of csrc/conv_wino4.hip / conv_h2.hip recorded from the launch
    ladders those files had before wino4_pick / h2_pick existed: the list of cases.  A case is a dict of the file's `fields` (the
    descriptor's varying fields; a `*_ptr` field is 0 for a null pointer, else 1 + the bytes its address is off alignment; `extra` is a dict
    of further raw descriptor fields, null for a null descriptor), `switches`, `cus`, `rc` and on rc == 0 `out`, named by `out_fields`
    (the kernel's template arguments, the launch grid, the dynamic-LDS bytes, the planned geometry)."""
    import json
    with open(os.path.join(GOLDEN, name + '.json')) as f:
        data = json.load(f)
    nf, ns = len(data['fields']), len(data['switch_fields'])
    cases = []
    for row in data['cases']:
        c = dict(zip(data['fields'], row[:nf]))
        c['switches'], c['cus'], c['rc'] = tuple(row[nf:nf + ns]), row[nf + ns], row[nf + ns + 1]
        c['out'] = tuple(row[nf + ns + 2:])
        c['named'] = dict(zip(data['out_fields'], c['out']))
        cases.append(c)
    return cases, data['out_fields']


_PICK_PTRS = ('out', 'res', 'dact_z', 'bias', 'mod', 'ln', 'w_wino4', 'w_wino4_zp', 'w_h2', 'x_amax')


def pick_dispatch_desc(c):
    """The sda_conv_desc of a load_pick_dispatch() case (None for the null descriptor): a planar 3 x 3 stride-1 launch unless `extra`
    says otherwise; pointer k of _PICK_PTRS is 0x100000 (k + 2) + its misalignment."""
    from sda_amd._lib import ConvDesc
    if c['extra'] is None:
        return None
    d = ConvDesc()
    d.x, d.w = 0x100000, 0x80000
    d.n, d.cx, d.cctx, d.hs, d.ws, d.ho, d.wo = c['n'], c['cx'], c.get('cctx', 0), c['hs'], c['ws'], c['ho'], c['wo']
    d.x_sc, d.x_sy, d.x_sx, d.x_sn_outer, d.n_inner = c['hs'] * c['ws'], c['ws'], 1, c['cx'] * c['hs'] * c['ws'], 1
    d.up_h = d.up_w = c['up']
    d.pool_h = d.pool_w = c['pool']
    d.zins_h = d.zins_w = c.get('zins', 1)
    d.stride_h = d.stride_w = c.get('stride', 1)
    d.kh = d.kw = 3
    d.cin_pad, d.cout, d.cout_pad, d.mt = c.get('cin_pad', c['cx']), c['cout'], c['cout'], 1
    d.act_in, d.act_d = c['act_in'], c['act_d']
    d.w_h2_scale, d.x_amax_static = c.get('w_h2_scale', 0.0), c.get('x_amax_static', 0.0)
    for k, name in enumerate(_PICK_PTRS):
        v = c.get(name + '_ptr', 0)
        for field in (('ln_mean', 'ln_rstd') if name == 'ln' else (name,)):
            setattr(d, field, 0x100000 * (k + 2) + v - 1 if v else None)
    for field, v in c['extra'].items():
        setattr(d, field, v)
    return d


# ---------------------------------------------------------------------------- model builders shared by GPU tests
def build_unet1d_tiny():
    import torch.nn as nn
    from sda_amd.score import MCScoreWrapper, ScoreUNet
    return MCScoreWrapper(ScoreUNet(3, embedding=8, hidden_channels=(8,), hidden_blocks=(1,), activation=nn.SiLU, spatial=1))


def build_unet1d_two_level():
    import torch.nn as nn
    from sda_amd.score import ScoreUNet
    return ScoreUNet(3, embedding=8, hidden_channels=(8, 16), hidden_blocks=(1, 2), activation=nn.SiLU, spatial=1)


def build_mcscore2d_tiny():
    import torch.nn as nn
    from sda_amd.experiments.kolmogorov import LocalScoreUNet
    from sda_amd.score import MCScoreNet
    net = MCScoreNet(2, order=1)
    net.kernel = LocalScoreUNet(channels=6, size=8, embedding=8, hidden_channels=(4, 8), hidden_blocks=(1, 1),
                                kernel_size=3, activation=nn.SiLU, spatial=2, padding_mode='circular')
    return net


def oracle_eps_from_module(module, kind, hidden=(128,) * 5):
    """An oracle (CPU) eps(x, t) sharing the weights of a sda_amd module."""
    from oracle import sda_oracle as O
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    if kind == 'mc2d':
        k = module.kernel
        net = k.network
        cfg = O.UNetConfig(net.in_channels, net.out_channels, net.mod_features, net.hidden_channels, net.hidden_blocks,
                           net.kernel_size[0], net.stride[0], 'SiLU', 2, 'circular')
        order = module.order

        def eps(x, t, dtype=None):
            s = sd if dtype is None else O.cast_sd(sd, dtype)
            kern = lambda xx, tt, c=None: O.score_unet(s, 'kernel.', cfg, xx, tt, s['kernel.forcing'])
            return O.mc_score_net(kern, order, x, t)
        return eps
    if kind == 'wrap1d':
        net = module.score.network
        cfg = O.UNetConfig(net.in_channels, net.out_channels, net.mod_features, net.hidden_channels, net.hidden_blocks,
                           net.kernel_size[0], net.stride[0], 'SiLU', 1, 'zeros')

        def eps(x, t, dtype=None):
            s = sd if dtype is None else O.cast_sd(sd, dtype)
            return O.mc_score_wrapper(lambda xx, tt, c=None: O.score_unet(s, 'score.', cfg, xx, tt, c), x, t)
        return eps
    if kind == 'local':                       # MCScoreNet over a ScoreNet / ResMLP kernel (experiments/lorenz/utils.py:45-59)
        k = module.kernel
        first = k.network[0]                  # Linear(features * window + embedding -> width)
        cfg = O.ResMLPConfig(first.in_features, module.kernel.network[-1][1].in_features if not isinstance(
            k.network[-1], torch.nn.Linear) else k.network[-1].out_features, tuple(hidden), 'SiLU')
        order = module.order

        def eps(x, t, dtype=None):
            s = sd if dtype is None else O.cast_sd(sd, dtype)
            kern = lambda xx, tt, c=None: O.score_net(s, 'kernel.', cfg, xx, tt, c)
            return O.mc_score_net(kern, order, x, t)
        return eps
    raise ValueError(kind)
