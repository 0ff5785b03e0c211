"""GPU: the adjoint of the Markov chains on the device -- ``sda_chain_advance_vjp`` and ``sda_chain_log_prob_grad`` against their
host replay (bit-equal where the arithmetic is +, -, x, / only), and the opt-in ``grad='device'`` route of ``sda_amd.chains`` and
``experiments.lorenz`` up to the two 4D-Vars against torch autograd through the torch-ops ``rk4`` on the CPU in float64
(tests/chain_vjp_util.py: the oracle, the bound, and what the bound requires of the inputs).  Every case prints its figures."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from sda_amd import _lib, chains, ops
from sda_amd.experiments import lorenz
from tests import chain_util as U
from tests import chain_vjp_util as V
from tests import launch_trace

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


def states_for(key, m):
    """(m, d) fp32: the fixture's states, repeated and nudged so that no two particles coincide."""
    x0 = V.x0_of(key)
    rng = np.random.default_rng(m)
    return (x0[np.arange(m) % len(x0)] + 0.01 * rng.standard_normal((m, x0.shape[1]))).astype(np.float32)


# ---------------------------------------------------------------- the kernels against their host replay
# m: 1, 7, and 257 = one particle into the second 256-thread workgroup.  Lorenz-96: sub-groups of 4 (64 particles per workgroup),
# 8 (32, n = 5 leaves three dead lanes each), 64 (4, n = 40 leaves 24 dead lanes; n = 64 none), m leaving the last workgroup partly filled.
@pytest.mark.parametrize('every', [False, True])
@pytest.mark.parametrize('key,m', [('l63', 1), ('l63', 7), ('l63', 257), ('l63_s3', 7), ('lv', 257), ('lv_s3', 7), ('l96_4', 70),
                                   ('l96_5', 37), ('l96_40', 6), ('l96_64', 5), ('l96_5_s3', 37)])
def test_vjp_kernel_equals_host_replay(dev, key, m, every):
    chain = V.make(key)
    model = chain.model()
    T = 3
    x = states_for(key, m)
    d = x.shape[1]
    g = V.cotangent((T, m, d) if every else (m, d), m + every)
    big = torch.full((m, d + 2), 7.0, device=dev)                      # x_in with a particle stride of d + 2
    big[:, :d] = torch.from_numpy(x).to(dev)
    xd = big[:, :d]
    states = torch.empty(T, m, d, device=dev)
    ops.chain_advance(model, xd, states, T, every=True, out_st=m * d)
    got = ops.chain_advance_vjp(model, xd, states, torch.from_numpy(g).to(dev), T, every)
    want = V.emu_vjp(chain, x, states.cpu().numpy(), g, T, every)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f'vjp {key} m={m} every={every}: |device - host replay| {err:.3e} of {np.abs(want).max():.3e}')
    if key.startswith('lv'):
        assert err <= 2 * ULP32 * np.abs(want).max()                   # expf: the libraries round differently
    else:
        assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.chain_advance_vjp(model, xd[:1], states[:, :1], torch.from_numpy(g).to(dev)[..., :1, :], T, every)[0], got[0])


@pytest.mark.parametrize('L', [2, 65, 66])
def test_log_prob_grad_kernel(dev, L):
    """b = 5: the fifth trajectory is the first wave of a second workgroup.  L = 65 / 66: index 64 takes r_63 from the previous stride,
    and at 66 it also owns a pair."""
    chain = chains.NoisyLorenz63(dt=0.025)
    x = V.noisy_trajectories(5, L)
    xd = torch.from_numpy(x).to(dev)
    value, grad = ops.chain_log_prob_grad(chain.model(), xd)
    assert torch.equal(value, ops.chain_log_prob(chain.model(), xd))
    hv, hg = V.emu_log_prob_grad(chain, x)
    assert np.array_equal(grad.cpu().numpy(), hg)
    assert np.abs(value.cpu().numpy() - hv).max() <= 1e-12 * np.abs(hv).max()          # (the sum's order differs: lanes, then a tree)
    r32, r64 = V.oracles(('lp', L, 5), V.log_prior_loss, x)
    V.check(f'device log_prob_grad L={L} b=5', grad, r32, r64)
    assert torch.equal(ops.chain_log_prob_grad(chain.model(), xd[:1])[1][0], grad[0])


# ---------------------------------------------------------------- autograd through chains.*(grad='device')
@pytest.mark.parametrize('key', ['l63', 'l63_s2', 'l96_5', 'l96_40', 'lv', 'l63_s3'])
@pytest.mark.parametrize('how', ['transition', 'every', 'last'])
def test_autograd_through_the_chain(dev, key, how):
    chain = V.make(key, grad='device')
    x0 = V.x0_of(key)
    T, every = (1, False) if how == 'transition' else (3, how == 'every')
    g = V.cotangent((T, *x0.shape) if every else x0.shape, 11 * T + every)
    xd = torch.from_numpy(x0).to(dev).requires_grad_()
    y = chain.transition(xd) if how == 'transition' else chain.trajectory(xd, T, last=not every)
    assert chains.LAST_CHAIN_GRAD_ROUTE == 'device' and y.requires_grad and y.shape == g.shape
    with torch.no_grad():
        same = chain.transition(xd) if how == 'transition' else chain.trajectory(xd, T, last=not every)
    assert torch.equal(y, same) and chains.LAST_CHAIN_GRAD_ROUTE is None      # forward is the no-grad launch, bitwise
    (y * torch.from_numpy(g).to(dev)).sum().backward()
    r32, r64 = V.oracles(('adv', key, T, every), V.advance_loss(V.make(key), T, every, g), x0)
    V.check(f'autograd {key} {how}', xd.grad, r32, r64)


@pytest.mark.parametrize('last', [False, True])
def test_autograd_through_the_noisy_chain(dev, last):
    """``last=True`` re-runs the forward in backward with the seed and first draw it kept: the recomputed states carry the same noise."""
    chain = chains.NoisyLorenz63(dt=0.025, grad='device')
    chain._draw = 5
    x0 = U.golden()['l63/x0']
    seed, T = 0x1234567890abcdef, 5
    g = V.cotangent((7, 3) if last else (T, 7, 3), 51 + last)
    xd = torch.from_numpy(x0).to(dev).requires_grad_()
    y = chain.trajectory(xd, T, last=last, seed=seed)
    assert chains.LAST_CHAIN_GRAD_ROUTE == 'device' and chain._draw == 10
    (y * torch.from_numpy(g).to(dev)).sum().backward()
    r32, r64 = V.oracles(('noisy-gpu', last), V.noisy_loss(chains.Lorenz63(dt=0.025), T, not last, g, seed, 0, 5), x0)
    V.check(f'autograd noisy trajectory last={last}', xd.grad, r32, r64)


def test_noisy_log_prob_takes_the_device_route(dev):
    x = V.noisy_trajectories(5, 9)
    chain = chains.NoisyLorenz63(dt=0.025, grad='device')
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    with launch_trace.trace() as calls:
        lp = chain.log_prob(xd[:, :-1], xd[:, 1:]).sum()
        lp.backward()
    names = [c[0] for c in calls]
    assert chains.LAST_CHAIN_GRAD_ROUTE == 'device' and names == ['sda_chain_advance', 'sda_chain_advance_vjp'], names
    r32, r64 = V.oracles(('lp', 9, 5), V.log_prior_loss, x)
    V.check('NoisyLorenz63.log_prob through moments', xd.grad, r32, r64)


def test_routes_that_stay_on_torch(dev):
    class Tweaked(chains.Lorenz63):
        def f(self, x):
            return super().f(x) * 1.0

    x0 = V.x0_of('l63')
    g = V.cotangent((3, *x0.shape), 11 * 3 + 1)
    r32, r64 = V.oracles(('adv', 'l63', 3, True), V.advance_loss(V.make('l63'), 3, True, g), x0)
    cases = {'float64 input': (chains.Lorenz63(grad='device'), torch.float64), "user's own f": (Tweaked(grad='device'), torch.float32),
             "grad='torch'": (chains.Lorenz63(), torch.float32)}
    for name, (chain, dtype) in cases.items():
        xd = torch.from_numpy(x0).to(dev, dtype).requires_grad_()
        chains.LAST_CHAIN_GRAD_ROUTE = None
        y = chain.trajectory(xd, 3)
        assert chains.LAST_CHAIN_GRAD_ROUTE == 'torch', name
        (y * torch.from_numpy(g).to(dev, dtype)).sum().backward()
        V.check(f'torch route, {name}', xd.grad, r32, r64)
    big = chains.Lorenz96(n=65, grad='device')
    assert big.transition(torch.randn(2, 65, device=dev).requires_grad_()).requires_grad and chains.LAST_CHAIN_GRAD_ROUTE == 'torch'
    # first order only
    chain = chains.Lorenz63(grad='device')
    xs = torch.from_numpy(x0).to(dev).requires_grad_()
    first, = torch.autograd.grad(chain.transition(xs).sum(), xs, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
    with pytest.raises(ValueError):
        chains.Lorenz96(grad='nonsense')


# ---------------------------------------------------------------- experiments.lorenz
def test_log_prior(dev):
    """A weight on every trajectory's value: the one multiply by the upstream cotangent shows."""
    x = V.noisy_trajectories(5, 66)
    w = np.array([1.0, -2.0, 0.5, 3.0, 0.25])
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    with launch_trace.trace() as calls:
        value = lorenz.log_prior(xd, grad='device')
        (value * torch.from_numpy(w).to(dev, value.dtype)).sum().backward()
    assert [c[0] for c in calls] == ['sda_chain_log_prob_grad'] and chains.LAST_CHAIN_GRAD_ROUTE == 'device'
    with torch.no_grad():
        assert torch.equal(value.detach(), lorenz.log_prior(xd))        # bitwise the no-grad kernel route
    chain = chains.NoisyLorenz63(dt=0.025)
    loss = lambda t: (chain.log_prob(t[:, :-1], t[:, 1:]).sum(-1) * torch.from_numpy(w).to(t.dtype)).sum()
    r32, r64 = V.oracles('log_prior weighted', loss, x)
    V.check('log_prior(grad=device) b=5 L=66', xd.grad, r32, r64)
    with pytest.raises(ValueError):
        lorenz.log_prior(xd, grad='nonsense')


A_OBS = lambda x: chains.Lorenz63.preprocess(x)[..., :1]                # the reference's observation of the Lorenz experiment


def _weak_loss(x, x_b, y, grad):
    return (x[0] - x_b.to(x)).square().sum() - lorenz.log_prior(x, grad=grad) - lorenz.log_likelihood(y.to(x), x, A_OBS, 0.05, 2)


def _weak_problem():
    truth = V.noisy_trajectories(1, 9, seed=7)[0]                       # (9, 3)
    rng = np.random.default_rng(8)
    x = (truth + 0.3 * rng.standard_normal(truth.shape)).astype(np.float32)
    y = A_OBS(torch.from_numpy(truth[::2])) + 0.05 * torch.from_numpy(rng.standard_normal((5, 1)).astype(np.float32))
    return x, y


def test_weak_4d_var(dev):
    x, y = _weak_problem()
    xd, yd = torch.from_numpy(x).to(dev), y.to(dev)
    x0 = xd.clone().requires_grad_()
    first = _weak_loss(x0, xd[0], yd, 'device')
    first.backward()
    first = first.detach()
    assert chains.LAST_CHAIN_GRAD_ROUTE == 'device'
    r32, r64 = V.oracles('weak', lambda t: _weak_loss(t, torch.from_numpy(x[0]), y, 'torch'), x)
    V.check('weak_4d_var first gradient', x0.grad, r32, r64)
    for grad in ('device', 'torch'):
        chains.LAST_CHAIN_GRAD_ROUTE = None
        out = lorenz.weak_4d_var(xd, yd, A_OBS, 0.05, 2, iterations=4, grad=grad)
        assert chains.LAST_CHAIN_GRAD_ROUTE == grad and out.shape == xd.shape and not out.requires_grad
        with torch.no_grad():
            final = _weak_loss(out, xd[0], yd, 'torch')
        print(f'weak_4d_var grad={grad}: objective {float(first):.6e} -> {float(final):.6e}')
        assert torch.isfinite(final) and float(final) < float(first)


def _strong_loss(chain, x0, x_b, y, A, length, step):
    return (x0 - x_b.to(x0)).square().sum() + ((y.to(x0) - A(chain.trajectory(x0, length)[::step])).square() / 0.05 ** 2).sum()


@pytest.mark.parametrize('system', ['lorenz63', 'lorenz96'])
def test_strong_4d_var(dev, system):
    if system == 'lorenz63':
        make, A, truth = (lambda **kw: chains.Lorenz63(dt=0.025, **kw)), A_OBS, U.golden()['l63/x0'][0]
    else:
        make, A, truth = (lambda **kw: chains.Lorenz96(n=8, dt=0.025, **kw)), (lambda x: x[..., ::2]), U.golden()['l96_5/x0'][0, [0, 1, 2, 3, 4, 0, 1, 2]]
    cpu = make()
    step, length = 2, 8
    rng = np.random.default_rng(9)
    x_b = (truth + 0.1 * rng.standard_normal(truth.shape)).astype(np.float32)
    with torch.no_grad():
        frames, t = [], torch.from_numpy(truth)
        for _ in range(length):
            t = cpu._rk4_transition(t)
            frames.append(t)
        y = A(torch.stack(frames)[::step])
    xb_d, y_d = torch.from_numpy(x_b).to(dev), y.to(dev)
    x0 = xb_d.clone().requires_grad_()
    first = _strong_loss(make(grad='device'), x0, xb_d, y_d, A, length, step)
    first.backward()
    first = first.detach()
    assert chains.LAST_CHAIN_GRAD_ROUTE == 'device'
    r32, r64 = V.oracles(('strong', system), lambda t: _strong_loss(cpu, t, torch.from_numpy(x_b), y, A, length, step), x_b)
    V.check(f'strong_4d_var first gradient {system}', x0.grad, r32, r64)
    for grad in ('device', 'torch'):
        chains.LAST_CHAIN_GRAD_ROUTE = None
        chain = None if (grad, system) == ('device', 'lorenz63') else make(grad=grad)       # None: the default chain
        out = lorenz.strong_4d_var(xb_d, y_d, A, 0.05, step, iterations=4, chain=chain)
        assert chains.LAST_CHAIN_GRAD_ROUTE == grad and out.shape == xb_d.shape and not out.requires_grad
        with torch.no_grad():
            final = _strong_loss(make(), out, xb_d, y_d, A, length, step)
        print(f'strong_4d_var {system} grad={grad}: objective {float(first):.6e} -> {float(final):.6e}')
        assert torch.isfinite(final) and float(final) < float(first)


def test_default_route_is_unchanged(dev):
    """No ``grad`` argument: the closure launches no kernel of this package (torch autograd through the torch-ops rk4, as before the
    option existed) and the result is bitwise that of the recipe written out."""
    x, y = _weak_problem()
    xd, yd = torch.from_numpy(x).to(dev), y.to(dev)
    with launch_trace.trace() as calls:
        got = lorenz.weak_4d_var(xd, yd, A_OBS, 0.05, 2, iterations=2)
    assert calls == [] and chains.LAST_CHAIN_GRAD_ROUTE == 'torch'
    chain = chains.NoisyLorenz63(dt=0.025)
    p = torch.nn.Parameter(xd.clone())
    optimizer = torch.optim.LBFGS((p,))

    def closure():
        optimizer.zero_grad()
        # the terms in the order weak_4d_var forms them: autograd adds the four contributions to p.grad in the order of the graph
        loss = ((p[0] - xd[0]).square().sum() - chain.log_prob(p[..., :-1, :], p[..., 1:, :]).sum(dim=-1)
                - Normal(yd, 0.05).log_prob(A_OBS(p[..., ::2, :])).sum(dim=(-1, -2)))
        loss.backward()
        return loss

    for _ in range(2):
        optimizer.step(closure)
    assert torch.equal(got, p.data)


def test_reference_recipe_after_install_as_sda():
    """The reference's own ``log_prior`` formula, with the chain it builds taken from ``sda.mcs`` after
    ``install_as_sda(native_chains=True)``: a chain built with grad='device' sends it through the kernels.  A process of its own,
    because the installation rebinds modules."""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import torch, sda_amd\n'
            'sda_amd.install_as_sda(native_chains=True)\n'
            'from sda.mcs import *\n'
            'from sda_amd import chains\n'
            'chain = NoisyLorenz63(dt=0.025, grad="device")\n'
            'x = chain.prior((2, 6)).cuda().requires_grad_()\n'
            'log_prior = chain.log_prob(x[..., :-1, :], x[..., 1:, :]).sum(dim=-1)\n'
            'log_prior.sum().backward()\n'
            'print("ROUTE", chains.LAST_CHAIN_GRAD_ROUTE, bool(torch.isfinite(x.grad).all()), tuple(x.grad.shape))\n')
    env = {k: v for k, v in os.environ.items() if k != 'SDA_MCS_FILE'}
    out = subprocess.run([sys.executable, '-B', '-c', code % ROOT], capture_output=True, text=True, env=env, cwd='/', timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['ROUTE', 'device', 'True', '(2,', '6,', '3)'], out.stdout
