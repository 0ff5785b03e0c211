"""GPU: the adjoint of the Kolmogorov flow on the device -- ``kflow_explicit_vjp_kernel``, the projection as its own adjoint, the
transition schedule, and ``KolmogorovFlow(grad='device')`` up to ``strong_4d_var`` -- against torch autograd of the torch-ops route
on the CPU in float64, with its float32 run as the yardstick (tests/kflow_vjp_ref.py).

Tolerance rule, as in test_gpu_kflow.py: 4 x the float32 oracle's own deviation from the float64 oracle, floored at 4 eps32
max|ref64| (``kflow_ref.bound``).  The limiter's derivative jumps at a = 0 and r = 0, so every case also requires of its INPUTS that
the oracle's own deviation stays below 1e-4 max|ref64| (``kflow_vjp_ref.bound_and_own``): no near-tie that the two precisions
resolve differently.  Each case prints its figures; with ``$SDA_KFLOW_PARITY`` set they are appended to that file
(profiles/kflow_vjp_parity.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains, ops
from sda_amd.experiments import kolmogorov
from tests import kflow_ref as R
from tests import kflow_vjp_ref as V

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


def record(case, own, err, bound):
    line = f'{case}: own {own:.3e} device {err:.3e} bound {bound:.3e}'
    print(line)
    path = os.environ.get('SDA_KFLOW_PARITY')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def check(case, got, ref32, ref64):
    b, own = V.bound_and_own(ref32, ref64)
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref64).max())
    record(case, own, err, b)
    assert err <= b, (case, err, b)


def model_for(n, dev, steps=1):
    f64 = R.Flow(n, 0.2)
    return ops.kflow_model(n, steps, float(f64.delta), float(f64.nu), dev)


def batch3(n, kind):
    """Three fields (3, 2, n, n) fp32: prior draws, or the ties field at three dyadic scales (its ties stay exact)."""
    if kind == 'ties':
        return R.ties_field(n)[None] * np.array([1.0, 2.0, 0.5], dtype=np.float32)[:, None, None, None]
    return V.prior_field(n, n, (3,))


def strided(a, dev):
    """`a` (3, ...) as the slice big[::2] of a larger device tensor whose other rows hold something else."""
    big = torch.full((6, *a.shape[1:]), 7.0, device=dev)
    big[::2] = torch.from_numpy(a).to(dev)
    return big[::2]


def cpu_chain(size=32, dt=0.2):
    """The oracle: the default chain, whose CPU tensors that require grad take the torch route in their own precision."""
    return chains.KolmogorovFlow(size=size, dt=dt)


def oracles(key, fn, x, g):
    """Computed once per key and shared."""
    if key not in _CACHE:
        _CACHE[key] = V.oracles(fn, x, g)
    return _CACHE[key]


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize('kind', ['prior', 'ties'])
@pytest.mark.parametrize('n', [16, 48, 272])
def test_explicit_vjp(dev, n, kind):
    """n = 16: one tile, every halo of 3 wraps into the tile itself; 48: 3 x 3 tiles; 272: 17 tiles per side."""
    x, g = batch3(n, kind), V.cotangent((3, 2, n, n), n + 1)
    model = model_for(n, dev)
    xd, gd = strided(x, dev), strided(g, dev)
    assert not xd.is_contiguous()
    got = ops.kflow_explicit_vjp(model, xd, gd)
    r32, r64 = oracles(('explicit', n, kind), V.chain_for(n)._torch_explicit, x, g)
    check(f'explicit vjp n={n} {kind}', got, r32, r64)
    if kind == 'ties':
        check(f'explicit vjp n={n} ties, host restatement', got, V.explicit_vjp(R.Flow(n, 0.2, dtype=np.float32), x, g), r64)
    assert torch.equal(ops.kflow_explicit_vjp(model, xd.contiguous(), gd.contiguous()), got)
    assert torch.equal(ops.kflow_explicit_vjp(model, xd[1], gd[1]), got[1])


@pytest.mark.parametrize('n', [16, 48])
def test_projection_is_its_own_adjoint(dev, n):
    g = V.cotangent((2, n, n), n)
    x = V.prior_field(n, n)                                            # the projection is linear: where it is taken does not matter
    r32, r64 = oracles(('project', n), V.chain_for(n)._torch_project, x, g)
    check(f'project as adjoint n={n}', ops.kflow_project(model_for(n, dev), torch.from_numpy(g).to(dev)), r32, r64)


@pytest.mark.parametrize('n', [16, 48])
def test_one_substep_vjp(dev, n):
    x, g = V.prior_field(n, n + 2, (2,)), V.cotangent((2, 2, n, n), n + 3)
    r32, r64 = oracles(('substep', n), V.chain_for(n, steps=1)._torch_transition, x, g)
    got = ops.kflow_transition_vjp(model_for(n, dev), torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev))
    check(f'substep vjp n={n}', got, r32, r64)


# ---------------------------------------------------------------- the chain
def test_whole_transition(dev):
    """Size 32, dt 0.2: 11 sub-steps, batch 2 -- the recompute slab and the backward walk with more than one state."""
    chain = chains.KolmogorovFlow(size=32, dt=0.2, grad='device')
    assert chain.steps == 11
    x, w = V.prior_field(32, 21, (2,)), V.cotangent((2, 2, 32, 32), 22)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    y = chain.transition(xd)
    assert chains.LAST_KFLOW_GRAD_ROUTE == 'device' and y.requires_grad
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    r32, r64 = oracles('transition', cpu_chain().transition, x, w)
    check('transition vjp n=32 (11 sub-steps)', xd.grad, r32, r64)


@pytest.mark.parametrize('last', [False, True])
def test_trajectory(dev, last):
    """Length 3 with a weight on every kept frame: a frame cotangent added at the wrong transition shows."""
    chain = chains.KolmogorovFlow(size=32, dt=0.2, grad='device')
    x = V.prior_field(32, 23, (2,))
    w = V.cotangent((2, 2, 32, 32) if last else (3, 2, 2, 32, 32), 24)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    y = chain.trajectory(xd, 3, last=last)
    assert y.shape == w.shape and chains.LAST_KFLOW_GRAD_ROUTE == 'device'
    with torch.no_grad():
        assert torch.equal(y, chain.trajectory(xd, 3, last=last))      # forward is the no-grad kernel route, bitwise
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    r32, r64 = oracles(('trajectory', last), lambda t: cpu_chain().trajectory(t, 3, last=last), x, w)
    check(f'trajectory vjp n=32 length 3 last={last}', xd.grad, r32, r64)


def test_trajectory_through_an_observation(dev):
    chain = chains.KolmogorovFlow(size=32, dt=0.2, grad='device')
    x = V.prior_field(32, 25)
    w = V.cotangent((3, 2, 16, 16), 26)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    A = lambda t: chains.KolmogorovFlow.coarsen(chain.trajectory(t, 3), 2)
    (A(xd) * torch.from_numpy(w).to(dev)).sum().backward()
    cpu = cpu_chain()
    r32, r64 = oracles('coarsen', lambda t: chains.KolmogorovFlow.coarsen(cpu.trajectory(t, 3), 2), x, w)
    check('coarsen(trajectory) vjp n=32', xd.grad, r32, r64)


def test_semantics(dev):
    chain = chains.KolmogorovFlow(size=32, dt=0.2, grad='device')
    x = torch.from_numpy(V.prior_field(32, 27, (3,))).to(dev)
    w = torch.from_numpy(V.cotangent((3, 2, 32, 32), 28)).to(dev)

    def grad_of(xs, ws):
        xs = xs.clone().requires_grad_()
        y = chain.transition(xs)
        return y, torch.autograd.grad((y * ws).sum(), xs)[0]

    y, g = grad_of(x, w)
    assert chains.LAST_KFLOW_GRAD_ROUTE == 'device'
    assert torch.equal(y, chain.transition(x)) and chains.LAST_KFLOW_GRAD_ROUTE is None
    assert torch.equal(grad_of(x, w)[1], g)                            # run to run
    assert torch.equal(grad_of(x[:1], w[:1])[1][0], g[0])              # whatever the batch
    # routes
    default = chains.KolmogorovFlow(size=32, dt=0.2)
    assert default.transition(x[0].clone().requires_grad_()).requires_grad and chains.LAST_KFLOW_GRAD_ROUTE == 'torch'
    unserved = chains.KolmogorovFlow(size=20, dt=0.01, grad='device')
    x20 = torch.from_numpy(V.prior_field(20, 29)).to(dev).requires_grad_()
    assert unserved.transition(x20).requires_grad and chains.LAST_KFLOW_GRAD_ROUTE == 'torch'
    with torch.no_grad():
        chain.transition(x.clone().requires_grad_())
    assert chains.LAST_KFLOW_GRAD_ROUTE is None
    # first order only
    xs = x[0].clone().requires_grad_()
    first, = torch.autograd.grad(chain.transition(xs).sum(), xs, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
    with pytest.raises(ValueError):
        chains.KolmogorovFlow(size=32, dt=0.2, grad='nonsense')


# ---------------------------------------------------------------- 4D-Var
def _loss_4d_var(chain, x0, x_b, y):
    x_b, y = x_b.to(x0), y.to(x0)
    return (x0 - x_b).square().sum() + (y - chains.KolmogorovFlow.coarsen(chain.trajectory(x0, 3), 2)).square().sum()


def test_strong_4d_var(dev):
    """Size 32, L = 3, A = coarsen(., 2), from a perturbed background.  Iterates are not compared between routes: L-BFGS amplifies
    rounding."""
    chain = chains.KolmogorovFlow(size=32, dt=0.2, grad='device')
    truth = V.prior_field(32, 31)
    x_b = (truth + 0.1 * V.cotangent(truth.shape, 32)).astype(np.float32)
    cpu = cpu_chain()
    with torch.no_grad():                                              # the observations: three frames of the truth, coarsened
        frames, t = [], torch.from_numpy(truth)
        for _ in range(3):
            t = cpu._torch_transition(t)
            frames.append(t)
        y = chains.KolmogorovFlow.coarsen(torch.stack(frames), 2)
    xb_d, y_d = torch.from_numpy(x_b).to(dev), y.to(dev)
    # the first closure: the loss at x0 = x_b
    x0 = xb_d.clone().requires_grad_()
    first = _loss_4d_var(chain, x0, xb_d, y_d)
    first.backward()
    first = first.detach()
    assert chains.LAST_KFLOW_GRAD_ROUTE == 'device'
    r32, r64 = oracles('4dvar', lambda t: _loss_4d_var(cpu, t, torch.from_numpy(x_b), y), x_b, np.ones(()))
    check('strong_4d_var first gradient n=32', x0.grad, r32, r64)
    A = lambda t: chains.KolmogorovFlow.coarsen(t, 2)
    chains.LAST_KFLOW_GRAD_ROUTE = None
    x = kolmogorov.strong_4d_var(xb_d, y_d, A, iterations=4, chain=chain)
    assert chains.LAST_KFLOW_GRAD_ROUTE == 'device' and x.shape == xb_d.shape and not x.requires_grad
    with torch.no_grad():
        final = _loss_4d_var(chain, x, xb_d, y_d)
    print(f'strong_4d_var: loss {float(first):.4e} -> {float(final):.4e}')
    assert torch.isfinite(final) and float(final) < float(first)
