"""GPU: the whole-net training kernels of the single-level 1-D U-Net (csrc/net1d_train.hip; training.parameter_gradients(net1d=True)):
forward / backward parity with the sampling kernels, the stored cotangents, the one-launch weight gradient, the one-launch pack, whole-net
gradients against the float64 oracle, launch counts and the switch."""
import ctypes

import pytest
import torch

from oracle import sda_oracle as O
from sda_amd import _lib, ops, training
from sda_amd._lib import Net1dDesc, Net1dTrainDesc
from tests import net1d_train_ref as R
from tests.util import build_unet1d_tiny, load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


def _case(circular, n, length, cin, c, cout, nb, tiles):
    return dict(circular=circular, n=n, len=length, cin=cin, c=c, cout=cout, nb=nb, tiles=tiles, act=1, unbiased=1, per_image=True,
                channel_last=True)


# the smallest shapes that reach each tiling of net1d_tiling (asserted through sda_net1d_tiles in _raw)
CASES = {
    'many_tiles': _case(False, 2, 64, 3, 64, 3, 6, 16),           # nf = 2, tp = 4: 16 tiles per sequence
    'whole_seq': _case(False, 300, 65, 3, 64, 3, 6, 1),           # one tile per sequence although len > any tile's own run
    'wrap_ragged': _case(True, 3, 38, 3, 64, 3, 6, 10),           # circular wrap across tiles, last tile 2 of 4 positions
    'tiny': _case(False, 6, 16, 3, 8, 3, 2, 1),                   # the shape of the golden net unet1d_tiny
    'c48_nb0': _case(False, 4, 50, 5, 48, 5, 0, 2),
}


class _Raw:
    """A random net at the C ABI: torch-layout weights, their packings (sda_net1d_pack), input, modulation rows."""

    def __init__(self, cfg, dev, seed=0):
        g = torch.Generator().manual_seed(seed)
        n, L, cin, c, cout, nb = cfg['n'], cfg['len'], cfg['cin'], cfg['c'], cfg['cout'], cfg['nb']
        self.cfg, self.dev = cfg, dev
        shapes = [(c, cin)] + [(c, c)] * (2 * nb) + [(cout, c)]
        self.ws = [(torch.randn(o, i, 3, generator=g) / (3 * i) ** 0.5).to(dev) for o, i in shapes]
        self.bs = [(0.1 * torch.randn(o, generator=g)).to(dev) for o, _ in shapes]
        self.x = torch.randn(n, L, cin, generator=g).to(dev).permute(0, 2, 1)                    # a (B, L, C) trajectory
        self.mod = (0.5 * torch.randn(n, max(nb, 1) * c, generator=g)).to(dev)
        self.cot = torch.randn(n, L, cout, generator=g).to(dev).permute(0, 2, 1)
        nconv = len(shapes)
        self.wf, self.wb = (torch.empty(nconv, 3 * 64 * 64, device=dev) for _ in range(2))
        self.bias = torch.empty(nconv, 64, device=dev)
        ops.net1d_pack(R.pack_desc(self.ws, self.bs, cin, c, cout, cin, self.wf, self.wb, self.bias))

    def desc(self, backward):
        cfg = self.cfg
        d = Net1dDesc()
        d.n, d.len, d.c, d.nblocks = cfg['n'], cfg['len'], cfg['c'], cfg['nb']
        d.circular, d.act, d.unbiased, d.eps = int(cfg['circular']), cfg['act'], cfg['unbiased'], 1e-5
        d.cin, d.cout = (cfg['cout'], cfg['cin']) if backward else (cfg['cin'], cfg['cout'])
        d.w, d.bias = (self.wb if backward else self.wf).data_ptr(), None if backward else self.bias.data_ptr()
        for k in range(cfg['nb']):
            d.mod[k] = self.mod[:, k * cfg['c']:].data_ptr()
        d.mod_sn = self.mod.stride(0)
        assert _lib.load().sda_net1d_tiles(ctypes.byref(d)) == cfg['tiles'], 'the planner moved this case to another tiling'
        return d

    def saves(self):
        cfg = self.cfg
        n, L, c, nb = cfg['n'], cfg['len'], cfg['c'], max(cfg['nb'], 1)
        nan = lambda *s: torch.full(s, float('nan'), device=self.dev)
        return dict(a=nan(nb, n, c, L), z=nan(nb, n, c, L), mean=nan(nb, n, L), rstd=nan(nb, n, L))

    @staticmethod
    def _io(d, x, out):
        d.x, d.x_sn, d.x_sc, d.x_sx = x.data_ptr(), x.stride(0), x.stride(1), x.stride(2)
        d.out, d.out_sn, d.out_sc, d.out_sx = out.data_ptr(), out.stride(0), out.stride(1), out.stride(2)

    def _set_saves(self, d, s):
        cfg = self.cfg
        d.a_save, d.z_save, d.save_stride = s['a'].data_ptr(), s['z'].data_ptr(), cfg['n'] * cfg['c'] * cfg['len']
        d.mean_save, d.rstd_save, d.stat_stride = s['mean'].data_ptr(), s['rstd'].data_ptr(), cfg['n'] * cfg['len']

    def forward(self, train):
        cfg, lib = self.cfg, _lib.load()
        d, s = self.desc(False), self.saves()
        out = torch.full((cfg['n'], cfg['len'], cfg['cout']), float('nan'), device=self.dev).permute(0, 2, 1)
        self._io(d, self.x, out)
        self._set_saves(d, s)
        if not train:
            _lib.check(lib.sda_net1d_fwd(ctypes.byref(d), ops._stream()), 'sda_net1d_fwd')
            return out, s
        t = Net1dTrainDesc()
        t.net = d
        s['tail_in'] = torch.full((cfg['n'], cfg['c'], cfg['len']), float('nan'), device=self.dev)
        t.tail_in = s['tail_in'].data_ptr()
        ops.net1d_fwd_train(t)
        return out, s

    def backward(self, s, train):
        cfg, lib = self.cfg, _lib.load()
        n, L, c, nb = cfg['n'], cfg['len'], cfg['c'], cfg['nb']
        d = self.desc(True)
        gin = torch.full((n, L, cfg['cin']), float('nan'), device=self.dev).permute(0, 2, 1)
        self._io(d, self.cot, gin)
        self._set_saves(d, s)
        if not train:
            _lib.check(lib.sda_net1d_bwd(ctypes.byref(d), ops._stream()), 'sda_net1d_bwd')
            return gin, None, None
        t = Net1dTrainDesc()
        t.net = d
        g_save = torch.full((2 * nb + 1, n, c, L), float('nan'), device=self.dev)
        mod_part = torch.full((max(nb, 1), n, cfg['tiles'], c), float('nan'), device=self.dev)
        t.g_save, t.g_stride, t.mod_part, t.mod_tiles = g_save.data_ptr(), n * c * L, mod_part.data_ptr(), cfg['tiles']
        ops.net1d_bwd_train(t)
        return gin, g_save, mod_part

    def float64(self):
        """(out, cotangent of every convolution's output in forward order, parameter gradients, modulation gradient) in float64."""
        cfg = self.cfg
        c, nb = cfg['c'], cfg['nb']
        ws = [w.double().cpu().requires_grad_() for w in self.ws]
        bs = [b.double().cpu().requires_grad_() for b in self.bs]
        mod = self.mod.double().cpu().requires_grad_()
        mods = [mod[:, k * c:(k + 1) * c] for k in range(nb)]
        out, outs = R.net64(self.x.double().cpu(), ws, bs, mods, cfg['circular'], cfg['act'], 1e-5, cfg['unbiased'])
        out.backward(self.cot.double().cpu())
        gm = mod.grad[:, :nb * c].reshape(-1, nb, c).permute(1, 0, 2) if nb else torch.zeros(0, cfg['n'], c, dtype=torch.float64)
        return out.detach(), [o.grad for o in outs], [(w.grad, b.grad) for w, b in zip(ws, bs)], gm


@pytest.fixture(scope='module')
def raws(dev):
    """Every case's net, both forwards, both backwards and the float64 reference, computed once and left unchanged."""
    res = {}
    for i, (name, cfg) in enumerate(CASES.items()):
        raw = _Raw(cfg, dev, seed=20 + i)
        out0, s0 = raw.forward(False)
        out1, s1 = raw.forward(True)
        gin0, _, _ = raw.backward(s0, False)
        gin1, g_save, mod_part = raw.backward(s1, True)
        res[name] = dict(raw=raw, out0=out0, s0=s0, out1=out1, s1=s1, gin0=gin0, gin1=gin1, g_save=g_save, mod_part=mod_part,
                         ref=raw.float64())
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('name', list(CASES))
def test_forward_parity(raws, name):
    r = raws[name]
    cfg = r['raw'].cfg
    assert torch.equal(r['out0'], r['out1'])
    for k in ('a', 'z', 'mean', 'rstd'):
        if cfg['nb']:
            assert torch.equal(r['s0'][k], r['s1'][k]), k
            assert torch.isfinite(r['s1'][k]).all(), k
    # the tail's input: the last block's output, recomputed from the saves in float64
    raw, s = r['raw'], r['s1']
    if cfg['nb']:
        k = cfg['nb'] - 1
        z = s['z'][k].double().cpu()
        y = R.conv64(R.ACTS[cfg['act']](z), raw.ws[2 + 2 * k].double().cpu(), raw.bs[2 + 2 * k].double().cpu(), cfg['circular'])
        want = s['a'][k].double().cpu() + y
    else:
        want = R.conv64(raw.x.double().cpu(), raw.ws[0].double().cpu(), raw.bs[0].double().cpu(), cfg['circular'])
    assert torch.isfinite(s['tail_in']).all()
    assert rel_err(s['tail_in'].cpu(), want) <= 1e-6
    assert rel_err(r['out1'].cpu(), r['ref'][0]) <= 1e-4


@pytest.mark.parametrize('name', list(CASES))
def test_backward_parity_and_stored_cotangents(raws, name):
    r = raws[name]
    cfg = r['raw'].cfg
    nb = cfg['nb']
    assert torch.equal(r['gin0'], r['gin1'])
    cots = r['ref'][1]                                       # forward order: head, (conv1, conv2) per block, tail
    assert torch.isfinite(r['g_save']).all(), 'a position no tile owns was left unwritten'
    slots = [(2 * nb, 0)] + [(2 * k + 1, 1 + 2 * k) for k in range(nb)] + [(2 * k, 2 + 2 * k) for k in range(nb)]
    for slot, v in slots:
        got, ref = r['g_save'][slot].double().cpu(), cots[v]
        err = (got - ref).abs().max().item()
        assert err <= R.TOL * ref.abs().max().item(), f'slot {slot} (convolution {v}): {err:.3e} vs scale {ref.abs().max().item():.3e}'
    if nb:
        assert torch.isfinite(r['mod_part']).all()
        ref = r['ref'][3]
        err = (r['mod_part'].sum(2).double().cpu() - ref).abs().max().item()
        assert err <= R.TOL * ref.abs().max().item(), f'modulation sums: {err:.3e}'


def _device_wgrad(t, slabs=0, frozen=()):
    lib = _lib.load()
    return R.run_wgrad(t, lib.sda_net1d_wgrad_work_floats, lambda d: lib.sda_net1d_wgrad(ctypes.byref(d), ops._stream()), slabs, frozen)


@pytest.mark.parametrize('name', list(CASES))
def test_wgrad_on_the_kernels_own_saves(raws, name):
    """sda_net1d_wgrad on what sda_net1d_fwd_train / sda_net1d_bwd_train left behind: every gradient of the net against float64 autograd."""
    r = raws[name]
    raw, s = r['raw'], r['s1']
    t = dict(cfg=raw.cfg, x=raw.x, gout=raw.cot, a=s['a'], z=s['z'], mean=s['mean'], rstd=s['rstd'], mod=raw.mod, tail_in=s['tail_in'],
             g_save=r['g_save'], mod_part=r['mod_part'])
    R.check_against((r['ref'][2], r['ref'][3]), _device_wgrad(t), what=name)


@pytest.mark.parametrize('name', list(CASES))
def test_wgrad_standalone_random_saved(dev, name):
    cfg = dict(CASES[name], per_image=name != 'tiny')         # (one case with a shared modulation row)
    t = R.random_saved(cfg, dev, seed=3)
    ref = R.reference_grads(t)
    base = _device_wgrad(t)
    R.check_against(ref, base, what=name)
    again = _device_wgrad(t)
    for x, y in zip(base[0] + base[1] + [base[2]], again[0] + again[1] + [again[2]]):
        assert torch.equal(x, y)
    for slabs in (1, 64):
        R.check_against(ref, _device_wgrad(t, slabs), what=f'{name} slabs {slabs}')
    nconv = 2 + 2 * cfg['nb']
    part = _device_wgrad(t, frozen=(0, nconv - 1))
    for v in range(1, nconv - 1):
        assert torch.equal(part[0][v], base[0][v]) and torch.equal(part[1][v], base[1][v])
    assert torch.equal(part[2], base[2])


def test_pack_parity(dev):
    for name in ('many_tiles', 'c48_nb0', 'tiny'):
        cfg = CASES[name]
        raw = _Raw(cfg, dev, seed=5)
        nconv = len(raw.ws)
        wf, wb = (torch.empty(nconv, 3 * 64 * 64, device=dev) for _ in range(2))
        bias = torch.zeros(nconv, 64, device=dev)
        for v, w in enumerate(raw.ws):
            ops.pack_conv_weight(w, w.shape[0], w.shape[1], 1, 3, False, w.shape[1], wf[v], 64, 64)
            bias[v, :w.shape[0]] = raw.bs[v]
        keep = 2
        for s, v in enumerate(reversed(range(nconv))):
            w = raw.ws[v]
            ops.pack_conv_weight(w, w.shape[0], w.shape[1], 1, 3, True, keep if v == 0 else w.shape[1], wb[s], 64, 64)
        wb1 = torch.empty_like(wb)
        ops.net1d_pack(R.pack_desc(raw.ws, raw.bs, cfg['cin'], cfg['c'], cfg['cout'], keep, None, wb1, None))
        assert torch.equal(raw.wf, wf) and torch.equal(raw.bias, bias) and torch.equal(wb1, wb)


# ------------------------------------------------------------------------------------------------ whole nets through the engine

def _tiny(dev):
    _, grp = load_golden('unet1d_tiny')
    net = build_unet1d_tiny()
    net.load_state_dict(grp['sd'])
    return net.to(dev), O.UNetConfig(3, 3, 8, (8,), (1,), 3, 2, 'SiLU', 1, 'zeros'), (16, 3)


def _global(dev):
    from sda_amd.experiments.lorenz import make_global_score
    torch.manual_seed(0)
    return make_global_score().to(dev), O.UNetConfig(3, 3, 32, (64,), (3,), 3, 2, 'SiLU', 1, 'zeros'), (32, 3)


def _wrapper_eps(cfg):
    return lambda sd, xt, t: O.mc_score_wrapper(lambda a, b, c=None: O.score_unet(sd, 'score.', cfg, a, b, c), xt, t)


@pytest.mark.parametrize('which,weighted', [('tiny', False), ('global', False), ('global', True)])
def test_whole_net_gradients_match_float64_oracle(dev, which, weighted):
    from tests.test_gpu_training import _check_net
    net, cfg, shape = (_tiny if which == 'tiny' else _global)(dev)
    torch.manual_seed(7)
    x = torch.randn(6, *shape, device=dev)
    w = (torch.rand(6, shape[0], 1, device=dev) + 0.5) if weighted else None
    calls = []
    orig = ops.net1d_wgrad
    ops.net1d_wgrad = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        _check_net(net, shape, _wrapper_eps(cfg), x, w, dev, net1d=True)
    finally:
        ops.net1d_wgrad = orig
    assert calls, 'the whole-net route did not run'


def _grads(net, shape, x, dev, seed, **switch):
    from tests.test_gpu_training import _hip_grads
    _, g, _, _ = _hip_grads(net, shape, x, None, seed, dev, **switch)
    return {k: v.clone() for k, v in g.items()}


def test_bitwise_reproducible_and_close_to_the_per_layer_route(dev):
    net, _, shape = _global(dev)
    torch.manual_seed(8)
    x = torch.randn(16, *shape, device=dev)
    g1, g2 = _grads(net, shape, x, dev, 21, net1d=True), _grads(net, shape, x, dev, 21, net1d=True)
    layers = _grads(net, shape, x, dev, 21)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert rel_err(g1[k], layers[k]) <= 1e-5, (k, rel_err(g1[k], layers[k]))


def _count(monkeypatch, names):
    seen = {n: 0 for n in names}
    for n in names:
        orig = getattr(ops, n)

        def wrap(*a, _n=n, _o=orig, **k):
            seen[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(ops, n, wrap)
    return seen


def test_launch_count_and_repack(dev, monkeypatch):
    from sda_amd import engine as E
    from sda_amd.score import VPSDE
    net, _, shape = _global(dev)
    sde = VPSDE(net, shape=shape).to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    torch.manual_seed(9)
    x = torch.randn(64, *shape, device=dev)
    seen = _count(monkeypatch, ['net1d_fwd_train', 'net1d_bwd_train', 'net1d_wgrad', 'net1d_pack', 'net1d_launch', 'conv_wgrad', 'plane_sum',
                                'block1d_fwd', 'block1d_bwd', 'pack_conv_weight', 'conv_igemm'])
    convs = []
    orig_lc = E.launch_conv
    monkeypatch.setattr(E, 'launch_conv', lambda *a, **k: (convs.append(1), orig_lc(*a, **k))[1])
    with training.parameter_gradients(net1d=True):
        for step in range(2):
            for k in seen:
                seen[k] = 0
            sde.loss(x).backward()
            assert (seen['net1d_fwd_train'], seen['net1d_bwd_train'], seen['net1d_wgrad']) == (1, 1, 1), seen
            assert seen['net1d_pack'] == 2, seen             # one per direction: the first step packs, every later one re-packs
            assert not any(seen[k] for k in ('net1d_launch', 'conv_wgrad', 'plane_sum', 'block1d_fwd', 'block1d_bwd', 'pack_conv_weight',
                                             'conv_igemm')) and not convs, (seen, len(convs))
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
            opt.step()
            opt.zero_grad()
        # no update in between: the packings are kept
        for k in seen:
            seen[k] = 0
        sde.loss(x).backward()
        assert seen['net1d_pack'] == 2                       # (the optimizer stepped after the last backward)
        for k in seen:
            seen[k] = 0
        sde.loss(x).backward()
        assert seen['net1d_pack'] == 0 and seen['net1d_fwd_train'] == 1


def test_sgd_trajectory_matches_float64_oracle(dev):
    """A few SGD steps on the device and on the float64 oracle from the same batches and draws: the packed-weight caches see each update."""
    from sda_amd.score import VPSDE
    net, cfg, shape = _tiny(dev)
    names = [k for k, _ in net.named_parameters()]
    sd64 = {k: v.detach().double().cpu().clone() for k, v in net.state_dict().items()}
    sde = VPSDE(net, shape=shape).to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    sched = O.Schedule()
    eps = _wrapper_eps(cfg)
    gen = torch.Generator().manual_seed(9)
    for step in range(5):
        x = torch.randn(4, *shape, generator=gen).to(dev)
        torch.manual_seed(100 + step)
        with training.parameter_gradients(net1d=True):
            sde.loss(x).backward()
        opt.step()
        opt.zero_grad()
        torch.manual_seed(100 + step)
        t = torch.rand(4, device=dev).double().cpu()
        e = torch.randn(4, *shape, device=dev).double().cpu()
        leaves = {k: sd64[k].clone().requires_grad_(k in names) for k in sd64}
        xt = sched.mu(t.reshape(-1, 1, 1)) * x.double().cpu() + sched.sigma(t.reshape(-1, 1, 1)) * e
        loss = (eps(leaves, xt, t) - e).square().mean()
        for k, gr in zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])):
            sd64[k] = sd64[k] - 0.05 * gr
    params = dict(net.named_parameters())
    for k in names:
        assert (params[k].detach().double().cpu() - sd64[k]).abs().max().item() <= 1e-4 * sd64[k].abs().max().item(), k
    xq, tq = torch.randn(3, *shape, generator=gen), torch.rand(3, generator=gen)
    with torch.no_grad():
        got = net(xq.to(dev), tq.to(dev)).cpu()
    assert rel_err(got, eps(sd64, xq.double(), tq.double())) <= 1e-4


def test_the_switch_off_changes_nothing(dev):
    """Sampling outputs and the guided VJP are bit-identical with the switch on or off; with it off, training is the per-layer route."""
    net, _, shape = _global(dev)
    torch.manual_seed(3)
    x = torch.randn(5, *shape, device=dev)
    t = torch.rand(5, device=dev)

    def sample_and_vjp():
        with torch.no_grad():
            out = net(x, t)
        xr = x.clone().requires_grad_()
        with training.input_only():
            gx, = torch.autograd.grad(net(xr, t).square().sum(), xr)
        return out, gx
    base = sample_and_vjp()
    with training.parameter_gradients(net1d=True):
        on = sample_and_vjp()
    for a, b in zip(base, on):
        assert torch.equal(a, b)
    seen = []
    orig = ops.net1d_fwd_train
    ops.net1d_fwd_train = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        g_off, g_off2 = _grads(net, shape, x, dev, 4), _grads(net, shape, x, dev, 4)
    finally:
        ops.net1d_fwd_train = orig
    assert not seen
    for k in g_off:
        assert torch.equal(g_off[k], g_off2[k]), k
