"""GPU: opt-in parameter gradients of the score U-Net (sda_amd.training, csrc/conv_wgrad.hip).

Per layer: the device weight-gradient kernel against float64 torch.autograd for every loader variant.  Whole net: the gradients
of ``VPSDE.loss(x, w).backward()`` against torch.autograd of the oracle's float64 ``score_unet`` on the same t / eps draws;
bitwise reproducibility, chunked / recomputed backward, an SGD trajectory against the oracle, ``utils.loop`` and the
untouched sampling VJP."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import sda_oracle as O
from sda_amd import engine as E
from sda_amd import ops, training
from sda_amd._lib import load as load_lib
from tests.util import build_mcscore2d_tiny, build_unet1d_two_level, load_golden, rel_err
from tests.wgrad_ref import make_case, reference, wgrad_desc, work_floats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def device_wgrad(case, dev, slabs=0, accumulate=False, dw=None, db=None, with_db=True):
    """One launch on the device: dw / db start NaN-filled unless given; ``work`` is NaN-filled, so an unwritten slab shows."""
    lib = load_lib()
    cout, cin, kh, kw = case['cout'], case['v64'].shape[1], case['kh'], case['kw']
    dw = torch.full((cout, cin, kh, kw), float('nan'), device=dev) if dw is None else dw
    db = torch.full((cout,), float('nan'), device=dev) if db is None else db
    dbp = db if with_db else None
    work = torch.full((work_floats(lib, wgrad_desc(case, dw, dbp, slabs=slabs, accumulate=accumulate)),), float('nan'), device=dev)
    d = wgrad_desc(case, dw, dbp, work, slabs=slabs, accumulate=accumulate)
    assert lib.sda_conv_wgrad(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize('width', [32, 64, 96, 192, 384])
@pytest.mark.parametrize('kind', ['conv1', 'conv1_shared', 'conv2', 'tail_up', 'head_s2', 'head0_ctx', 'head0_window', 'tail10'])
def test_layer_wgrad_matches_float64(dev, kind, width):
    cin, cout = width, width
    if kind == 'tail10':
        cout = 10
    elif kind == 'head0_ctx':
        cin = 11
    elif kind == 'tail_up':
        cin = min(2 * width, 384)
    elif kind == 'head_s2':
        cin = max(width // 2, 32)
    h = 8 if width >= 192 else 16
    case = make_case(kind, dev, cin=cin, cout=cout, n=2, h=h, w=h, circular=width != 64, seed=width)
    dw, db = device_wgrad(case, dev)
    rw, rb = reference(case)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dw, rw), rel_err(db, rb))


@pytest.mark.parametrize('kind', ['conv1', 'conv2', 'tail_up', 'head_s2', 'plain'])
def test_layer_wgrad_odd_1d_and_slabs(dev, kind):
    for case, slabs in ((make_case(kind, dev, cin=7, cout=33, n=3, h=7, w=9, circular=kind != 'head_s2', seed=1), 0),
                        (make_case(kind, dev, cin=64, cout=64, n=4, w=32, one_d=True, seed=2), 0),
                        (make_case(kind, dev, cin=24, cout=40, n=3, h=12, w=12, seed=3), 3)):
        dw, db = device_wgrad(case, dev, slabs)
        rw, rb = reference(case)
        assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5


def test_plane_sum(dev):
    x, y = torch.randn(3, 5, 7, 9, device=dev), torch.randn(3, 5, 7, 9, device=dev)
    out = torch.full((3, 8), float('nan'), device=dev)
    ops.plane_sum(x, y, out[:, 2:], 8, False, False)
    want = (x - y).double().sum(dim=(2, 3))
    assert rel_err(out[:, 2:7], want) <= 1e-6
    tot = torch.zeros(1, 5, device=dev)
    ops.plane_sum(x, y, tot, 0, True, True)
    assert rel_err(tot[0], want.sum(0)) <= 1e-6


def _check_layer(case, dev, slabs=0):
    dw, db = device_wgrad(case, dev, slabs)
    rw, rb = reference(case)
    assert rel_err(dw, rw) <= 1e-5 and rel_err(db, rb) <= 1e-5, (rel_err(dw, rw), rel_err(db, rb))
    return dw, db


def test_layer_wgrad_accumulates_onto_a_prior(dev):
    case = make_case('conv1', dev, cin=8, cout=8, n=2, h=6, w=6, seed=8)
    dw, db = device_wgrad(case, dev)
    gen = torch.Generator().manual_seed(80)
    pw, pb = (torch.randn(dw.shape, generator=gen) * 5).to(dev), (torch.randn(db.shape, generator=gen) * 5).to(dev)
    dw2, db2 = device_wgrad(case, dev, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, pw + dw) and torch.equal(db2, pb + db)


def test_layer_wgrad_without_bias_leaves_the_buffer_alone(dev):
    # no bias gradient asked for: nothing may land behind dw, where a bias buffer (NaN-filled) sits
    case = make_case('plain', dev, cin=4, cout=4, n=1, h=4, w=4)
    buf = torch.full((4 * 4 * 9 + 4,), float('nan'), device=dev)
    dw, db = device_wgrad(case, dev, dw=buf[:144].view(4, 4, 3, 3), db=buf[144:], with_db=False)
    assert torch.isnan(buf[144:]).all()
    assert rel_err(dw, reference(case)[0]) <= 1e-5


@pytest.mark.parametrize('act', ['ReLU', 'ELU', 'GELU', 'SELU'])
def test_layer_wgrad_conv2_activations(dev, act):
    _check_layer(make_case('conv2', dev, cin=24, cout=40, n=2, h=10, w=12, act=act, seed=13), dev)


def test_layer_wgrad_slab_override(dev):
    case = make_case('conv1', dev, cin=10, cout=70, n=4, h=16, w=16, seed=7)       # 1024 positions: 32 stages
    for slabs in (1, 2, 7, 64):
        dw, db = _check_layer(case, dev, slabs)
        dw2, db2 = device_wgrad(case, dev, slabs)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), slabs


@pytest.mark.parametrize('cin', [1, 43])
@pytest.mark.parametrize('cout', [97, 100, 130])
def test_layer_wgrad_ragged_four_tile(dev, cout, cin):
    # cout > 96 and not a multiple of 32: the 128-cout tile with a ragged last tile
    _check_layer(make_case('plain', dev, cin=cin, cout=cout, n=2, h=9, w=7, circular=cin == 1, seed=cout + cin), dev)
    if cin > 1:
        _check_layer(make_case('conv1', dev, cin=cin, cout=cout, n=3, h=6, w=10, seed=cout), dev)


@pytest.mark.parametrize('ksize', [(5, 5), (1, 7), (3, 5)])
@pytest.mark.parametrize('circular', [True, False])
def test_layer_wgrad_kernel_sizes(dev, ksize, circular):
    for kind in ('conv1', 'tail_up', 'head_s2'):
        _check_layer(make_case(kind, dev, cin=12, cout=33, n=2, h=8, w=10, ksize=ksize, circular=circular, seed=sum(ksize)), dev)


@pytest.mark.parametrize('ksize,pad', [((3, 3), (0, 0)), ((2, 2), (1, 0)), ((3, 3), (2, 1)), ((4, 5), (3, 0)), ((1, 2), (0, 1))])
def test_layer_wgrad_explicit_pad(dev, ksize, pad):
    for circular in (True, False):
        _check_layer(make_case('conv2', dev, cin=9, cout=20, n=2, h=8, w=6, ksize=ksize, pad=pad, circular=circular, seed=sum(pad)), dev)
        _check_layer(make_case('head_s2', dev, cin=9, cout=20, n=2, h=8, w=6, ksize=ksize, pad=pad, circular=circular, seed=sum(pad)), dev)


@pytest.mark.parametrize('n_off', [1, 2, 3])
def test_layer_wgrad_window_source_with_image_offset(dev, n_off):
    # the MC window view (two windows per trajectory) read from window n_off on: what a recomputed chunk hands the head
    _check_layer(make_case('head0_window', dev, cin=6, cout=16, h=8, w=8, n_off=n_off, seed=n_off), dev)


def test_layer_wgrad_long_contraction(dev):
    """One Kolmogorov training layer: conv1 (modulation + LayerNorm), 96 -> 96, 32 images of 64 x 64, circular: 131 072 positions
    summed in fp32.  The bound is 4 x the error plain float32 torch.autograd on the CPU makes on the same case against the same
    float64 reference (an independent fp32 evaluation; the factor allows for a different summation tree).

    Measured on an MI355X (relative to max |ref|): float32 CPU autograd dw 1.79e-6, db 2.74e-6 (16 threads; 2.83e-6 / 4.03e-6 on another
    host); the device kernel dw 8.70e-7, db 1.03e-6 -- it also meets the 1e-5 of the small layers, and the host emulator gives the same
    two figures."""
    case = make_case('conv1', dev, cin=96, cout=96, n=32, h=64, w=64, circular=True, seed=96)
    dw, db = device_wgrad(case, dev)
    rw, rb = reference(case)
    a, mod = case['keep'][0].cpu(), case['keep'][1].cpu()
    v32 = O.layer_norm(a + mod[:, :, None, None], dim=1)
    assert v32.dtype == torch.float32
    W = torch.zeros(96, 96, 3, 3, requires_grad=True)
    b = torch.zeros(96, requires_grad=True)
    cw, cb = torch.autograd.grad(O._conv(v32, W, b, 2, (1, 1), 'circular'), (W, b), case['g'].cpu())
    yard_w, yard_b = rel_err(cw, rw), rel_err(cb, rb)
    err_w, err_b = rel_err(dw, rw), rel_err(db, rb)
    print(f'long contraction: float32 CPU autograd dw {yard_w:.3e} db {yard_b:.3e}; device dw {err_w:.3e} db {err_b:.3e}')
    assert err_w <= 4 * yard_w and err_b <= 4 * yard_b, (err_w, yard_w, err_b, yard_b)


@pytest.mark.parametrize('hw', [(1, 1), (5, 51), (16, 16), (257, 1), (64, 64)])
def test_plane_sum_plane_sizes(dev, hw):
    # 1, 255, 256, 257 and 4096 elements per plane: below, at and beyond one pass of the 256 threads
    gen = torch.Generator().manual_seed(hw[0])
    x, y = torch.randn(3, 5, *hw, generator=gen).to(dev), torch.randn(3, 5, *hw, generator=gen).to(dev)
    want = (x - y).double().sum(dim=(2, 3))
    out = torch.full((3, 9), float('nan'), device=dev)              # rows of out_sn = 9 > c floats, written from column 3 on
    ops.plane_sum(x, y, out[:, 3:], 9, False, False)
    assert rel_err(out[:, 3:8], want) <= 1e-6
    assert torch.isnan(out[:, :3]).all() and torch.isnan(out[:, 8:]).all()
    ops.plane_sum(x, None, out[:, 3:], 9, False, True)              # y = None, added onto what is there
    assert rel_err(out[:, 3:8], want + x.double().sum(dim=(2, 3))) <= 1e-6
    assert torch.isnan(out[:, :3]).all() and torch.isnan(out[:, 8:]).all()
    tot = torch.full((1, 7), float('nan'), device=dev)              # shared row: write, then accumulate a second batch
    ops.plane_sum(x, y, tot[:, 1:], 0, True, False)
    assert rel_err(tot[0, 1:6], want.sum(0)) <= 1e-6
    ops.plane_sum(y, None, tot[:, 1:], 0, True, True)
    assert rel_err(tot[0, 1:6], want.sum(0) + y.double().sum(dim=(0, 2, 3))) <= 1e-6
    assert torch.isnan(tot[0, 0]) and torch.isnan(tot[0, 6])


def _load_fuzz(name):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz', name + '.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


def test_wgrad_fuzz_sample(dev):
    """The 60 draws of test_wgrad_emulator.test_wgrad_fuzz_sample on the device (tests/fuzz/wgrad_fuzz.py), each within 1e-5 of
    float64; the largest |device - emulator| / max |ref| over the sample is printed and goes into any failure message (not asserted:
    the accumulation order inside the MFMA is not documented to equal the emulator's fmaf chain)."""
    import random
    from tests.test_wgrad_emulator import FUZZ_CASES, FUZZ_SEED
    fuzz = _load_fuzz('wgrad_fuzz')
    device, emu = fuzz.device(), fuzz.emulator()
    rng = random.Random(FUZZ_SEED)
    bad, gap = [], 0.0
    for i in range(FUZZ_CASES):
        spec = fuzz.draw_case(rng, i)
        dw, db, msg = fuzz.run_case(spec, device)
        if msg is None:
            ref = fuzz.reference(spec)
            ew, eb = fuzz.errors(spec, dw, db, ref)
            if not (torch.isfinite(dw).all() and ew <= fuzz.TOL and eb <= fuzz.TOL):
                msg = f'dw err {ew:.3e}, db err {eb:.3e}'
            edw, edb, emsg = fuzz.run_case(spec, emu)
            assert emsg is None, emsg
            gap = max(gap, (dw - edw).abs().max().item() / ref[2], 0.0 if db is None else (db - edb).abs().max().item() / ref[3])
        if msg:
            bad.append((i, msg, spec['cfg']))
    print(f'wgrad fuzz sample: max |device - emulator| / max |ref| = {gap:.3e}')
    assert not bad, f'max |device - emulator| / max |ref| = {gap:.3e}\n' + '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)


def test_train_fuzz_sample(dev):
    """A bounded sample of tests/fuzz/train_fuzz.py: 20 random nets (net_fuzz's architecture and shape draws, widths 32 / 64 / 96
    among them: the forward takes the Winograd kernels, the weight gradient reads the same saved activations), every parameter
    gradient and the input gradient in one backward; every second case through recomputed chunks of 2.  No case is skipped."""
    import random
    fuzz = _load_fuzz('train_fuzz')
    rng = random.Random(5)
    bad, widths = [], set()
    for i in range(20):
        cfg, msg = fuzz.one_case(rng, dev, 300 + i, chunk=2 if i % 2 else None, acts=fuzz.SMOOTH)
        widths.add(cfg['hidden'][0])
        if msg:
            bad.append((i, msg, cfg))
    assert not bad, '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)
    assert {32, 64, 96} <= widths, widths


# ------------------------------------------------------------------------------------------------------------ whole nets

def _oracle_grads(module, eps_fn, x, t, e, weight):
    """float64 grads of the denoising loss through the oracle net over the module's state dict -> {name: grad}."""
    sd = {k: v.detach().double().cpu().requires_grad_(k in dict(module.named_parameters())) for k, v in module.state_dict().items()}
    sched = O.Schedule()
    t64, e64, x64 = t.double().cpu(), e.double().cpu(), x.double().cpu()
    tb = t64.reshape((-1,) + (1,) * (x.dim() - 1))
    xt = sched.mu(tb) * x64 + sched.sigma(tb) * e64
    err = (eps_fn(sd, xt, t64) - e64).square()
    loss = err.mean() if weight is None else (err * weight.double().cpu()).mean() / weight.double().cpu().mean()
    names = [k for k, p in module.named_parameters()]
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    return loss.detach(), dict(zip(names, grads)), sd


def _hip_grads(module, shape, x, weight, seed, dev, **switch):
    """``switch``: keywords of ``training.parameter_gradients`` (none: the default route)."""
    from sda_amd.score import VPSDE
    sde = VPSDE(module, shape=shape).to(dev)
    module.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    with training.parameter_gradients(**switch):
        loss = sde.loss(x, w=weight)
        loss.backward()
    torch.manual_seed(seed)
    t = torch.rand(x.shape[0], dtype=x.dtype, device=dev)
    e = torch.randn_like(x)
    return loss.detach(), {k: p.grad for k, p in module.named_parameters()}, t, e


def _check_net(module, shape, eps_fn, x, weight, dev, seed=11, **switch):
    loss, g, t, e = _hip_grads(module, shape, x, weight, seed, dev, **switch)
    loss64, g64, _ = _oracle_grads(module, eps_fn, x, t, e, weight)
    assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
    for k, ref in g64.items():
        got = g[k]
        assert got is not None, f'{k}: no gradient formed'
        err = (got.double().cpu() - ref).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, f'{k}: {err:.3e} vs scale {ref.abs().max().item():.3e}'
    assert any('embedding' in k for k in g64) and any('project' in k for k in g64)


def _kernel_eps(cfg, prefix=''):
    return lambda sd, xt, t: O.score_unet(sd, prefix, cfg, xt, t, sd.get(prefix + 'forcing'))


def test_net_gradients_mcscore2d_tiny_kernel(dev):
    g, grp = load_golden('mcscore2d_tiny')
    mc = build_mcscore2d_tiny()
    mc.load_state_dict(grp['sd'])
    kernel = mc.kernel.to(dev)
    cfg = O.UNetConfig(7, 6, 8, (4, 8), (1, 1), 3, 2, 'SiLU', 2, 'circular')
    torch.manual_seed(3)
    x = torch.randn(5, 6, 8, 8, device=dev)
    w = torch.rand(5, 1, 8, 8, device=dev) + 0.5
    for weight in (None, w):
        _check_net(kernel, (6, 8, 8), _kernel_eps(cfg), x, weight, dev)


def test_net_gradients_mcscore2d_tiny_markov_chain(dev):
    # the fused window route of MCScoreNet (one trajectory: the time embedding broadcasts over its windows)
    g, grp = load_golden('mcscore2d_tiny')
    mc = build_mcscore2d_tiny()
    mc.load_state_dict(grp['sd'])
    mc = mc.to(dev)
    cfg = O.UNetConfig(7, 6, 8, (4, 8), (1, 1), 3, 2, 'SiLU', 2, 'circular')

    def eps_fn(sd, xt, t):
        kern = lambda xx, tt, c=None: O.score_unet(sd, 'kernel.', cfg, xx, tt, sd['kernel.forcing'])
        return O.mc_score_net(kern, 1, xt, t)
    torch.manual_seed(4)
    x = torch.randn(1, 5, 2, 8, 8, device=dev)
    _check_net(mc, (5, 2, 8, 8), eps_fn, x, None, dev)


def test_net_gradients_unet1d_two_level(dev):
    g, grp = load_golden('unet1d_two_level')
    net = build_unet1d_two_level()
    net.load_state_dict(grp['sd'])
    net = net.to(dev)
    cfg = O.UNetConfig(3, 3, 8, (8, 16), (1, 2), 3, 2, 'SiLU', 1, 'zeros')
    torch.manual_seed(5)
    x = torch.randn(6, 3, 32, device=dev)
    _check_net(net, (3, 32), _kernel_eps(cfg), x, torch.rand(6, 1, 32, device=dev) + 0.5, dev)


@pytest.mark.parametrize('widths,window', [((64, 128, 256), 3), ((96, 192, 384), 5)])
def test_net_gradients_kolmogorov(dev, widths, window):
    from sda_amd.experiments.kolmogorov import make_score
    torch.manual_seed(0)
    kernel = make_score(window=window, hidden_channels=widths).kernel.to(dev)
    cfg = O.UNetConfig(2 * window + 1, 2 * window, 64, widths, (3, 3, 3), 3, 2, 'SiLU', 2, 'circular')
    torch.manual_seed(6)
    x = torch.randn(2, 2 * window, 64, 64, device=dev)
    _check_net(kernel, (2 * window, 64, 64), _kernel_eps(cfg), x, None, dev)


def _tiny_kernel(dev):
    g, grp = load_golden('mcscore2d_tiny')
    mc = build_mcscore2d_tiny()
    mc.load_state_dict(grp['sd'])
    return mc.kernel.to(dev)


def test_gradients_bitwise_reproducible_and_chunked(dev, monkeypatch):
    kernel = _tiny_kernel(dev)
    torch.manual_seed(8)
    x = torch.randn(12, 6, 8, 8, device=dev)
    _, g1, _, _ = _hip_grads(kernel, (6, 8, 8), x, None, 21, dev)
    g1 = {k: v.clone() for k, v in g1.items()}
    _, g2, _, _ = _hip_grads(kernel, (6, 8, 8), x, None, 21, dev)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # keep nothing: every chunk recomputes its forward inside the backward, in chunks of a few images
    monkeypatch.setattr(E, 'KEEP_HBM_FRACTION', 1e-12)
    monkeypatch.setattr(E, 'CHUNK_HBM_FRACTION', 5 * kernel.network.engine().bytes_per_image(8, 8, True) /
                        torch.cuda.get_device_properties(dev).total_memory)
    _, g3, _, _ = _hip_grads(kernel, (6, 8, 8), x, None, 21, dev)
    for k in g1:
        assert rel_err(g3[k], g1[k]) <= 1e-6, (k, rel_err(g3[k], g1[k]))


def test_sgd_trajectory_matches_float64_oracle(dev):
    """Ten SGD steps on the device and on the float64 oracle from the same batches and draws; then the device forward with the
    updated weights equals the oracle's (the packed-weight caches re-packed after each step)."""
    from sda_amd.score import VPSDE
    kernel = _tiny_kernel(dev)
    cfg = O.UNetConfig(7, 6, 8, (4, 8), (1, 1), 3, 2, 'SiLU', 2, 'circular')
    names = [k for k, _ in kernel.named_parameters()]
    sd64 = {k: v.detach().double().cpu().clone() for k, v in kernel.state_dict().items()}
    sde = VPSDE(kernel, shape=(6, 8, 8)).to(dev)
    opt = torch.optim.SGD(kernel.parameters(), lr=0.05)
    sched = O.Schedule()
    gen = torch.Generator().manual_seed(9)
    for step in range(10):
        x = torch.randn(4, 6, 8, 8, generator=gen).to(dev)
        torch.manual_seed(100 + step)
        with training.parameter_gradients():
            sde.loss(x).backward()
        opt.step()
        opt.zero_grad()
        torch.manual_seed(100 + step)
        t = torch.rand(4, device=dev).double().cpu()
        e = torch.randn(4, 6, 8, 8, device=dev).double().cpu()
        leaves = {k: sd64[k].clone().requires_grad_(k in names) for k in sd64}
        xt = sched.mu(t.reshape(-1, 1, 1, 1)) * x.double().cpu() + sched.sigma(t.reshape(-1, 1, 1, 1)) * e
        loss = (O.score_unet(leaves, '', cfg, xt, t, leaves['forcing']) - e).square().mean()
        grads = torch.autograd.grad(loss, [leaves[k] for k in names])
        for k, gr in zip(names, grads):
            sd64[k] = sd64[k] - 0.05 * gr
    params = dict(kernel.named_parameters())
    for k in names:
        ref = sd64[k]
        assert (params[k].detach().double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), k
    xq = torch.randn(3, 6, 8, 8, generator=gen)
    tq = torch.rand(3, generator=gen)
    with torch.no_grad():
        got = kernel(xq.to(dev), tq.to(dev)).cpu()
    want = O.score_unet(sd64, '', cfg, xq.double(), tq.double(), sd64['forcing'])
    assert rel_err(got, want) <= 1e-4


def test_utils_loop_adamw(dev):
    from sda_amd.score import VPSDE
    from sda_amd.utils import loop
    kernel = _tiny_kernel(dev)
    sde = VPSDE(kernel, shape=(6, 8, 8)).to(dev)
    gen = torch.Generator().manual_seed(10)
    data = [(torch.randn(6, 8, 8, generator=gen), {}) for _ in range(8)]
    out = list(loop(sde, data, data[:4], epochs=3, batch_size=4, learning_rate=1e-3, scheduler='cosine', device=dev))
    assert len(out) == 3
    for epoch, (lt, lv, lr) in enumerate(out):
        assert torch.isfinite(torch.tensor([lt, lv])).all()
        assert abs(lr - 1e-3 * (1 + torch.cos(torch.tensor(torch.pi * epoch / 3)).item()) / 2) <= 1e-9
    assert not training.enabled()


def test_sampling_vjp_unchanged_by_switch(dev):
    from sda_amd.score import GaussianScore, VPSDE
    kernel = _tiny_kernel(dev)
    A = lambda x: x[..., ::2, ::2]
    torch.manual_seed(12)
    x = torch.randn(3, 6, 8, 8, device=dev)
    y = torch.randn(3, 6, 4, 4, device=dev)
    t = torch.tensor(0.4, device=dev)
    gs = GaussianScore(y, A=A, std=0.3, sde=VPSDE(kernel, shape=(6, 8, 8))).to(dev)
    off = gs(x, t).clone()
    with training.parameter_gradients():
        on = gs(x, t)
    assert torch.equal(on, off)
    assert all(p.grad is None for p in kernel.parameters())
