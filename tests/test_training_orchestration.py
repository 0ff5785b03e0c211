"""CPU: the Python orchestration of the training route (sda_amd.training) replayed on host tensors through tests/cpu_shim.py --
which tensor is saved for which layer, which cotangent meets which input, the image offset of recomputed chunks into the
source view / the modulation rows / the per-image context, and what adds into what -- against float64 torch.autograd through
the oracle.  Weight gradients run through the host replay of csrc/conv_wgrad.hip (same planner, loader and reduction order as
the device kernel).  Tolerance per tensor: 1e-4 of max |ref|, as tests/test_gpu_training.py uses on the device."""
import importlib.util
import os
import random

import pytest
import torch
import torch.nn as nn

from oracle import sda_oracle as O
from sda_amd import engine as E
from sda_amd import ops, training
from sda_amd.score import MCScoreNet, ScoreUNet, VPSDE
from tests import cpu_shim
from tests.util import build_mcscore2d_tiny, build_unet1d_tiny, build_unet1d_two_level, load_golden, rel_err

TOL = 1e-4


@pytest.fixture(autouse=True)
def shim(monkeypatch):
    cpu_shim.install(monkeypatch)
    yield


def _leaves(module):
    names = [k for k, _ in module.named_parameters()]
    sd = {k: v.detach().double().clone().requires_grad_(k in names) for k, v in module.state_dict().items()}
    return names, sd


def _assert_grads(got: dict, want: dict, tol=TOL):
    for k, ref in want.items():
        assert got.get(k) is not None, f'{k}: no gradient formed'
        err = (got[k].double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        assert err <= tol * scale + 1e-12, f'{k}: {err:.3e} vs scale {scale:.3e}'


# ------------------------------------------------------------------------------------------ VPSDE.loss(...).backward()

def _loss_grads(module, shape, x, weight, seed):
    sde = VPSDE(module, shape=shape)
    module.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    with training.parameter_gradients():
        loss = sde.loss(x, w=weight)
        loss.backward()
    torch.manual_seed(seed)                      # the draws of VPSDE.loss, replayed
    t = torch.rand(x.shape[0], dtype=x.dtype)
    e = torch.randn_like(x)
    return loss.detach(), {k: p.grad.clone() for k, p in module.named_parameters()}, t, e


def _oracle_loss_grads(module, eps_fn, x, t, e, weight):
    names, sd = _leaves(module)
    sched = O.Schedule()
    t64, e64, x64 = t.double(), e.double(), x.double()
    tb = t64.reshape((-1,) + (1,) * (x.dim() - 1))
    xt = sched.mu(tb) * x64 + sched.sigma(tb) * e64
    err = (eps_fn(sd, xt, t64) - e64).square()
    loss = err.mean() if weight is None else (err * weight.double()).mean() / weight.double().mean()
    return loss.detach(), dict(zip(names, torch.autograd.grad(loss, [sd[k] for k in names])))


def _check_loss(module, shape, eps_fn, x, weight, seed=11):
    loss, g, t, e = _loss_grads(module, shape, x, weight, seed)
    loss64, g64 = _oracle_loss_grads(module, eps_fn, x, t, e, weight)
    assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
    _assert_grads(g, g64)
    assert any('embedding' in k for k in g64) and any('project' in k for k in g64)


TINY2D = O.UNetConfig(7, 6, 8, (4, 8), (1, 1), 3, 2, 'SiLU', 2, 'circular')


def _kernel_eps(cfg, prefix=''):
    return lambda sd, xt, t: O.score_unet(sd, prefix, cfg, xt, t, sd.get(prefix + 'forcing'))


def _tiny_mc():
    g, grp = load_golden('mcscore2d_tiny')
    mc = build_mcscore2d_tiny()
    mc.load_state_dict(grp['sd'])
    return mc


def test_loss_gradients_mcscore2d_tiny_kernel():
    kernel = _tiny_mc().kernel
    torch.manual_seed(3)
    x = torch.randn(5, 6, 8, 8)
    w = torch.rand(5, 1, 8, 8) + 0.5
    for weight in (None, w):
        _check_loss(kernel, (6, 8, 8), _kernel_eps(TINY2D), x, weight)


def test_loss_gradients_mcscore2d_tiny_markov_chain():
    # the fused window route of MCScoreNet (one trajectory per sample: its time embedding broadcasts over the windows)
    mc = _tiny_mc()

    def eps_fn(sd, xt, t):
        kern = lambda xx, tt, c=None: O.score_unet(sd, 'kernel.', TINY2D, xx, tt, sd['kernel.forcing'])
        return O.mc_score_net(kern, 1, xt, t)
    torch.manual_seed(4)
    x = torch.randn(1, 5, 2, 8, 8)
    for weight in (None, torch.rand(1, 5, 1, 8, 8) + 0.5):
        _check_loss(mc, (5, 2, 8, 8), eps_fn, x, weight)


def test_loss_gradients_unet1d_two_level():
    g, grp = load_golden('unet1d_two_level')
    net = build_unet1d_two_level()
    net.load_state_dict(grp['sd'])
    cfg = O.UNetConfig(3, 3, 8, (8, 16), (1, 2), 3, 2, 'SiLU', 1, 'zeros')
    torch.manual_seed(5)
    x = torch.randn(6, 3, 32)
    for weight in (None, torch.rand(6, 1, 32) + 0.5):
        _check_loss(net, (3, 32), _kernel_eps(cfg), x, weight)


# ------------------------------------------------------------------------------------------ one backward of net(x, t[, c])

def _net_grads(net, x, t, c, g, need_x=True):
    """-> (out, {name: grad}) of one backward with the cotangent g; 'x' is the input gradient."""
    net.zero_grad(set_to_none=True)
    xs = x.clone().requires_grad_(need_x)
    with training.parameter_gradients():
        out = net(xs, t) if c is None else net(xs, t, c)
        out.backward(g)
    got = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    got['x'] = xs.grad
    return out.detach(), got


def _oracle_net_grads(net, eps_fn, x, t, c, g):
    names, sd = _leaves(net)
    xo = x.double().requires_grad_(True)
    out = eps_fn(sd, xo, t.double(), None if c is None else c.double())
    grads = torch.autograd.grad(out, [xo] + [sd[k] for k in names], g.double())
    return out.detach(), dict(zip(['x'] + names, grads))


def _check_net(net, eps_fn, x, t, c=None, seed=0):
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))
    out, got = _net_grads(net, x, t, c, g)
    ref, want = _oracle_net_grads(net, eps_fn, x, t, c, g)
    assert rel_err(out, ref) <= TOL
    _assert_grads(got, want)
    return got, want


def test_local_score_unet_forcing_reaches_the_head_gradient():
    from sda_amd.experiments.kolmogorov import LocalScoreUNet
    torch.manual_seed(20)
    net = LocalScoreUNet(channels=4, size=8, embedding=8, hidden_channels=(3, 6), hidden_blocks=(1, 2), kernel_size=3,
                         activation=nn.GELU, spatial=2, padding_mode='circular')
    cfg = O.UNetConfig(5, 4, 8, (3, 6), (1, 2), 3, 2, 'GELU', 2, 'circular')
    x, t = torch.randn(3, 4, 8, 8), torch.rand(3)
    got, want = _check_net(net, lambda sd, xx, tt, c: O.score_unet(sd, '', cfg, xx, tt, sd['forcing']), x, t)
    head = next(k for k, p in net.named_parameters() if p.dim() == 4 and p.shape[1] == 5)
    ref = want[head][:, 4]                       # the taps that read the forcing plane
    assert ref.abs().max() > 1e-3 * want[head].abs().max()
    assert (got[head][:, 4].double() - ref).abs().max() <= TOL * ref.abs().max()


def test_mc_score_wrapper_channel_last_source(monkeypatch):
    g, grp = load_golden('unet1d_tiny')
    net = build_unet1d_tiny()
    net.load_state_dict(grp['sd'])
    cfg = O.UNetConfig(3, 3, 8, (8,), (1,), 3, 2, 'SiLU', 1, 'zeros')
    seen, real = [], ops.conv_wgrad

    def spy(conv, *a, **k):
        seen.append((conv.cx, conv.x_sc, conv.x_sx))
        return real(conv, *a, **k)
    monkeypatch.setattr(ops, 'conv_wgrad', spy)
    torch.manual_seed(21)
    x, t = torch.randn(4, 12, 3), torch.rand(4)          # (B, L, C): the wrapper hands the U-Net a transposed view

    def eps_fn(sd, xx, tt, c):
        return O.mc_score_wrapper(lambda a, b, c=None: O.score_unet(sd, 'score.', cfg, a, b, c), xx, tt)
    _check_net(net, eps_fn, x, t)
    assert (3, 1, 3) in seen, f'no weight gradient read a channel-last source: {seen}'


def _unet2d(context=0, channels=3, act=nn.SiLU, pad='circular'):
    torch.manual_seed(30)
    net = ScoreUNet(channels, context, embedding=8, hidden_channels=(4, 8), hidden_blocks=(1, 1), kernel_size=3, activation=act,
                    spatial=2, padding_mode=pad)
    for p in net.parameters():
        p.data.mul_(1.5)
    cfg = O.UNetConfig(channels + context, channels, 8, (4, 8), (1, 1), 3, 2, act.__name__, 2, pad)
    return net, (lambda sd, xx, tt, c: O.score_unet(sd, '', cfg, xx, tt, c))


def test_width_32_net_needs_no_device_library(monkeypatch):
    # a 3 x 3 convolution 32 wide is one the second-generation Winograd kernel serves: the shim switches that form off, so that
    # packing the weights does not reach for the device library on a machine that has none
    from sda_amd import _lib

    def no_library():
        raise _lib.SdaHipError('the host replay must not load the device library')
    monkeypatch.setattr(_lib, 'load', no_library)
    torch.manual_seed(34)
    net = ScoreUNet(2, embedding=8, hidden_channels=(32,), hidden_blocks=(1,), kernel_size=3, activation=nn.SiLU, spatial=2,
                    padding_mode='circular')
    cfg = O.UNetConfig(2, 2, 8, (32,), (1,), 3, 2, 'SiLU', 2, 'circular')
    _check_net(net, lambda sd, xx, tt, c: O.score_unet(sd, '', cfg, xx, tt, c), torch.randn(2, 2, 4, 4), torch.rand(2))


def test_input_and_parameter_gradients_in_one_backward():
    net, eps_fn = _unet2d(context=1)
    torch.manual_seed(31)
    x, t, c = torch.randn(3, 3, 4, 8), torch.rand(3), torch.randn(3, 1, 4, 8)
    got, want = _check_net(net, eps_fn, x, t, c)
    assert got['x'] is not None and 'x' in want
    # ... and the parameter gradients do not depend on whether the input gradient is asked for
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(0))
    _, alone = _net_grads(net, x, t, c, g, need_x=False)
    assert alone['x'] is None
    for k in want:
        if k != 'x':
            assert torch.equal(alone[k], got[k]), k


def test_frozen_subset():
    net, eps_fn = _unet2d()
    torch.manual_seed(32)
    x, t = torch.randn(2, 3, 8, 8), torch.rand(2)
    g = torch.randn(x.shape)
    _, full = _net_grads(net, x, t, None, g)
    params = dict(net.named_parameters())
    convs = [k for k, p in params.items() if p.dim() == 4]
    frozen = {convs[0], convs[2], convs[2].replace('weight', 'bias'), next(k for k in params if 'project' in k and 'weight' in k),
              next(k for k in params if 'embedding' in k and 'bias' in k)}
    assert frozen <= set(params)
    for k in frozen:
        params[k].requires_grad_(False)
    _, part = _net_grads(net, x, t, None, g)
    for k in params:
        if k in frozen:
            assert part[k] is None, f'{k}: frozen, yet it has a gradient'
        else:
            assert torch.equal(part[k], full[k]), k
    assert torch.equal(part['x'], full['x'])


def test_two_backwards_accumulate():
    net, eps_fn = _unet2d()
    torch.manual_seed(33)
    xa, xb, t = torch.randn(2, 3, 8, 8), torch.randn(3, 3, 8, 8), torch.rand(())
    ga, gb = torch.randn(xa.shape), torch.randn(xb.shape)
    _, a = _net_grads(net, xa, t, None, ga)
    _, b = _net_grads(net, xb, t, None, gb)
    net.zero_grad(set_to_none=True)
    with training.parameter_gradients():
        net(xa, t).backward(ga)
        net(xb, t).backward(gb)
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, a[k] + b[k]), k


# ------------------------------------------------------------------------------------------ recomputed chunks

def _all_recomputed(k):
    return lambda self, n, hs, ws, save, device, fraction=None: min(n, k)


def _kept_head(keep, k):
    # forward_all asks with KEEP_HBM_FRACTION for what it may keep, and without a fraction for the recomputed chunks
    return lambda self, n, hs, ws, save, device, fraction=None: min(n, keep if fraction is not None else k)


CHUNKINGS = {'all_recomputed_2': (_all_recomputed(2), 9), 'kept_8_then_3': (_kept_head(8, 3), 18), 'ragged_3': (_all_recomputed(3), 10)}


def _chunk_case(source, n):
    """-> net, eps_fn, x, t, c with n images (windows) in the engine's batch."""
    gen = torch.Generator().manual_seed(40 + n)
    if source == 'mc_window':                    # B >= 2 trajectories of 3 / 5 / 9 windows: chunks of 2 or 3 straddle them
        B = 2 if n % 2 == 0 else 3
        nw = n // B
        assert B * nw == n and nw % 2 == 1 and nw % 3 != 1
        torch.manual_seed(41)
        net = MCScoreNet(2, order=1, embedding=8, hidden_channels=(4, 8), hidden_blocks=(1, 1), kernel_size=3, activation=nn.SiLU,
                         spatial=2, padding_mode='circular')
        for p in net.parameters():
            p.data.mul_(1.5)
        cfg = O.UNetConfig(6, 6, 8, (4, 8), (1, 1), 3, 2, 'SiLU', 2, 'circular')

        def eps_fn(sd, xx, tt, c):
            return O.mc_score_net(lambda a, b, _c=None: O.score_unet(sd, 'kernel.', cfg, a, b, None), 1, xx, tt)
        return net, eps_fn, torch.randn(B, nw + 2, 2, 4, 4, generator=gen), torch.rand(B, nw, generator=gen), None
    context = 2 if source == 'per_image_context' else 0
    net, eps_fn = _unet2d(context=context, pad='zeros' if source == 'shared_time' else 'circular')
    x = torch.randn(n, 3, 4, 4, generator=gen)
    t = torch.rand((), generator=gen) if source == 'shared_time' else torch.rand(n, generator=gen)
    c = torch.randn(n, context, 4, 4, generator=gen) if context else None
    return net, eps_fn, x, t, c


@pytest.mark.parametrize('source', ['per_image_time', 'shared_time', 'mc_window', 'per_image_context'])
@pytest.mark.parametrize('chunking', list(CHUNKINGS))
def test_chunked_training_backward(monkeypatch, chunking, source):
    chunk_size, n = CHUNKINGS[chunking]
    net, eps_fn, x, t, c = _chunk_case(source, n)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
    out0, whole = _net_grads(net, x, t, c, g)                    # (the shim keeps everything: one forward, one backward)
    calls = []
    real_fwd = E.UNetEngine.forward_chunk

    def fwd(self, src, lo, hi, *a, **k):
        calls.append((lo, hi))
        return real_fwd(self, src, lo, hi, *a, **k)
    monkeypatch.setattr(E.UNetEngine, 'forward_chunk', fwd)
    monkeypatch.setattr(E.UNetEngine, 'chunk_size', chunk_size)
    out1, got = _net_grads(net, x, t, c, g)
    # the route that was meant to run did run: chunk boundaries of the forward, then of the recomputing backward
    k = {'all_recomputed_2': 2, 'kept_8_then_3': 3, 'ragged_3': 3}[chunking]
    lo0 = 8 if chunking == 'kept_8_then_3' else 0
    rest = [(lo, min(n, lo + k)) for lo in range(lo0, n, k)]
    assert calls == ([(0, 8)] if lo0 else []) + rest + rest, calls
    assert torch.equal(out0, out1)
    ref, want = _oracle_net_grads(net, eps_fn, x, t, c, g)
    assert rel_err(out1, ref) <= TOL
    _assert_grads(got, want)
    unet = net.kernel.network if hasattr(net, 'kernel') else net.network
    conv_params = {id(p) for p in unet.engine().train_params()}
    assert len(conv_params) == 2 * len(unet.engine().convs())
    for name, p in net.named_parameters():           # the convolution gradients: each chunk added into the same buffers
        if id(p) in conv_params:
            assert rel_err(got[name], whole[name]) <= 1e-6, (name, rel_err(got[name], whole[name]))


# ------------------------------------------------------------------------------------------ random whole nets

def _train_fuzz():
    spec = importlib.util.spec_from_file_location(
        'train_fuzz', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz', 'train_fuzz.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


def test_train_fuzz_sample():
    """A bounded sample of tests/fuzz/train_fuzz.py on the host replay: random 1-D / 2-D nets of 1-3 levels, MC windows, context,
    shared or per-sample times; every parameter gradient and the input gradient in one backward, alternately unchunked and
    through recomputed chunks of 2 images.  Smooth activations only: no case is skipped."""
    fuzz = _train_fuzz()
    rng = random.Random(2024)
    bad = []
    for i in range(24):
        cfg, msg = fuzz.one_case(rng, 'cpu', i, chunk=2 if i % 2 else None, acts=fuzz.SMOOTH, small=True)
        if msg:
            bad.append((i, msg, cfg))
    assert not bad, '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)
