"""GPU: the Kolmogorov-flow kernels (sda_amd/csrc/kflow.hip) and ``sda_amd.chains.KolmogorovFlow`` against the NumPy restatement
tests/kflow_ref.py.

Tolerance rule for every "device vs float64 replay" comparison: the yardstick is the float32 replay's own deviation from the
float64 replay on the same input, the bound is 4 x that (the matrix-core transform sums in another order than np.fft), floored at
4 eps32 max|ref64| (``kflow_ref.bound``).  Each case prints its yardstick and the device error; with ``$SDA_KFLOW_PARITY`` set
they are appended to that file (profiles/kflow_parity.txt is such a record)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains, ops
from tests import kflow_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)
_FLOWS, _FIELDS = {}, {}


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


def flows(n, dt=0.2):
    if (n, dt) not in _FLOWS:
        _FLOWS[n, dt] = R.Flow(n, dt, dtype=np.float64), R.Flow(n, dt, dtype=np.float32)
    return _FLOWS[n, dt]


def field(n, kind):
    """fp32 test inputs, computed once: a prior draw of the replay, or the 'ties' field."""
    if (n, kind) not in _FIELDS:
        if kind == 'ties':
            _FIELDS[n, kind] = R.ties_field(n)
        else:
            z = np.random.default_rng(n).standard_normal((2, n, n))
            _FIELDS[n, kind] = flows(n)[0].prior(z).astype(np.float32)
    return _FIELDS[n, kind]


def record(case, own, err, bound):
    line = f'{case}: own {own:.3e} device {err:.3e} bound {bound:.3e}'
    print(line)
    path = os.environ.get('SDA_KFLOW_PARITY')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def check(case, got, ref32, ref64):
    b, own = R.bound(ref32, ref64)
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref64).max())
    record(case, own, err, b)
    assert err <= b, (case, err, b)


def one_step_model(n, dev, steps=1):
    f64 = flows(n)[0]
    return ops.kflow_model(n, steps, float(f64.delta), float(f64.nu), dev)


def max_div(x):
    """max |div| of a velocity pair, in float64 on the host."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(flows(x.shape[-1])[0].divergence(x)).max())


# ---------------------------------------------------------------- transform
@pytest.mark.parametrize('n', [16, 48, 256])
def test_hartley_transform(dev, n):
    """Hm x Hm against Re - Im of np.fft, and twice = the identity; batch 3 as a strided slice of a larger tensor."""
    big = torch.from_numpy(np.random.default_rng(n).standard_normal((6, n, n)).astype(np.float32)).to(dev)
    x = big[::2]
    xh = x.cpu().numpy()
    y = ops.kflow_hartley(x)
    ref64 = R.hartley2(xh.astype(np.float64))
    ref32 = R.hartley2(xh)
    check(f'hartley n={n}', y, ref32, ref64)
    check(f'hartley twice n={n}', ops.kflow_hartley(y), R.hartley2(ref32), xh.astype(np.float64))
    assert torch.equal(ops.kflow_hartley(x.contiguous()), y)
    g = torch.from_numpy(R.prior_filter(n).astype(np.float32)).to(dev)
    want = np.fft.ifft2(np.fft.fft2(xh.astype(np.float64)) * R.prior_filter(n)).real
    want32 = np.fft.ifft2(np.fft.fft2(xh) * R.prior_filter(n).astype(np.float32)).real.astype(np.float32)
    check(f'hartley filter n={n}', ops.kflow_hartley(ops.kflow_hartley(x, g)), want32, want)


# ---------------------------------------------------------------- explicit terms, projection, sub-step
@pytest.mark.parametrize('kind', ['prior', 'ties'])
@pytest.mark.parametrize('n', [16, 48, 272])
def test_explicit_terms_and_substep(dev, n, kind):
    """n = 16: one stencil tile, every halo wraps into it; 48: three stencil tiles per side, one partial 64-tile of the products;
    272: four full 64-tiles and a partial one."""
    f64, f32 = flows(n)
    x = field(n, kind)
    xd = torch.from_numpy(x).to(dev)
    model = one_step_model(n, dev)
    check(f'explicit n={n} {kind}', ops.kflow_explicit(model, xd), f32.explicit(x), f64.explicit(x))
    got = ops.kflow_advance(model, xd, 1)
    r32, r64 = f32.substep(x), f64.substep(x)
    check(f'substep n={n} {kind}', got, r32, r64)
    res, own = max_div(got.cpu().numpy()), max_div(r32)
    record(f'substep div n={n} {kind}', own, res, 4 * own)
    assert res <= 4 * own


@pytest.mark.parametrize('n', [16, 48])
def test_projection(dev, n):
    f64, f32 = flows(n)
    us = f32.explicit(field(n, 'prior'))                              # not divergence-free
    got = ops.kflow_project(one_step_model(n, dev), torch.from_numpy(us).to(dev))
    check(f'project n={n}', got, f32.project(us), f64.project(us))
    g = got.cpu().numpy().astype(np.float64)
    assert max_div(g) <= 4 * max_div(f32.project(us)) < max_div(us)
    # the gradient of a periodic potential has zero mean whatever the potential's own mean is
    drift = np.abs(g.mean(axis=(-2, -1)) - us.astype(np.float64).mean(axis=(-2, -1))).max()
    assert drift <= 4 * EPS * np.abs(us).max()


def test_laminar_state_stays(dev):
    """100 sub-steps at N = 64 from the discrete laminar fixed point: rounding accumulates at worst linearly, 4 eps32 A a step.
    No replay is involved unless the float32 replay itself drifts more; then the bound is 4 x its drift."""
    n = 64
    f64, f32 = flows(n)
    x, A = f32.laminar()
    out = ops.kflow_advance(one_step_model(n, dev, steps=100), torch.from_numpy(x).to(dev), 1).cpu().numpy()
    y = x
    for _ in range(100):
        y = f32.substep(y)
    own = float(np.abs(y.astype(np.float64) - x).max())
    drift = float(np.abs(out.astype(np.float64) - x).max())
    bound = max(100 * 4 * EPS * A, 4 * own)
    record('laminar 100 sub-steps n=64', own, drift, bound)
    assert drift <= bound


# ---------------------------------------------------------------- the chain
def test_chain_semantics_are_bitwise(dev):
    chain = chains.KolmogorovFlow(size=32, dt=0.2)
    x = chain.prior((4,), device=dev, seed=11)
    assert x.shape == (4, 2, 32, 32) and chain.steps == R.steps_for(32, 0.2)
    traj = chain.trajectory(x, 5)
    assert traj.shape == (5, 4, 2, 32, 32)
    y = x
    for t in range(5):
        y = chain.transition(y)
        assert torch.equal(y, traj[t]), t
    assert torch.equal(chain.trajectory(x, 5, last=True), traj[-1])
    assert torch.equal(chain.trajectory(x[2], 5), traj[:, 2])
    assert torch.equal(chain.trajectory(x, 5), traj)
    x23 = chain.prior((2, 3), device=dev, seed=12)
    t23 = chain.trajectory(x23, 2)
    assert t23.shape == (2, 2, 3, 2, 32, 32)
    assert torch.equal(t23[:, 1, 2], chain.trajectory(x23[1, 2], 2))
    assert torch.equal(chain.transition(x23), t23[0])
    assert torch.isfinite(traj).all()


def test_prior(dev):
    n, seed = 48, 1234
    chain = chains.KolmogorovFlow(size=n, dt=0.2)
    x = chain.prior((2,), device=dev, seed=seed)
    z = ops.randn_rows(torch.empty(2, 2, n, n, device=dev), seed, 0).cpu().numpy()
    f64, f32 = flows(n)
    r32 = f32.prior(z)
    check(f'prior n={n}', x, r32, f64.prior(z))
    xh = x.cpu().numpy().astype(np.float64)
    assert max_div(xh) <= 4 * max_div(r32)
    speed = np.sqrt(xh[:, 0] ** 2 + xh[:, 1] ** 2).max(axis=(-2, -1))
    assert np.abs(speed - 3).max() <= 1e-5 * 3
    assert torch.equal(chain.prior((2,), device=dev, seed=seed), x)
    assert not torch.equal(chain.prior((2,), device=dev, seed=seed + 1), x)
    assert not torch.equal(x[0], x[1])
    torch.manual_seed(3)
    a = chain.prior((), device=dev)
    torch.manual_seed(3)
    assert a.shape == (2, n, n) and torch.equal(chain.prior((), device=dev), a)
    # an empty shape is an empty batch; a device named without its index shares the tables of the current device
    assert chain.prior((0, 3), device=dev, seed=seed).shape == (0, 3, 2, n, n)
    assert torch.equal(chain.prior((2,), device='cuda', seed=seed), x) and len(chain._models) == len(chain._filters) == 1


def test_one_whole_transition_of_make_chain(dev):
    """Size 256, 82 sub-steps, batch 2: finite, divergence-free, and inside the envelope of the float32 replay of the same input
    widened by 10 % (one transition is far shorter than the flow's divergence time)."""
    from sda_amd.experiments import kolmogorov
    chain = kolmogorov.make_chain()
    x = chain.prior((2,), device=dev, seed=5)
    y = chain.transition(x)
    assert y.shape == x.shape and torch.isfinite(y).all()
    f32 = R.Flow(256, 0.2, dtype=np.float32)
    assert f32.steps == chain.steps == 82
    ref = f32.transition(x.cpu().numpy())
    yh = y.cpu().numpy().astype(np.float64)
    res, own = max_div(yh), max_div(ref)
    record('transition div n=256', own, res, 4 * own)
    assert res <= 4 * own
    for b in range(2):
        V = 1.1 * np.abs(ref[b]).max()
        E = 0.5 * (ref[b].astype(np.float64) ** 2).mean()
        e = 0.5 * (yh[b] ** 2).mean()
        print(f'field {b}: max|u| {np.abs(yh[b]).max():.4f} (replay {V / 1.1:.4f})  energy {e:.5f} (replay {E:.5f})')
        assert np.abs(yh[b]).max() <= V and 0.9 * E <= e <= 1.1 * E


def test_unserved_inputs_take_the_torch_route(dev):
    n = 20                                                             # 20 % 16 != 0
    chain = chains.KolmogorovFlow(size=n, dt=0.01)
    assert chain.steps == 1
    x = field(n, 'prior')
    f64, f32 = flows(n, 0.01)
    check('torch route n=20', chain.transition(torch.from_numpy(x).to(dev)), f32.transition(x), f64.transition(x))
    p = chain.prior((3,), device=dev, seed=2)
    z = ops.randn_rows(torch.empty(3, 2, n, n, device=dev), 2, 0).cpu().numpy()
    assert p.shape == (3, 2, n, n)
    check('prior n=20 (torch route)', p, R.Flow(n, 0.2, dtype=np.float32).prior(z), R.Flow(n, 0.2).prior(z))
    n = 16
    chain = chains.KolmogorovFlow(size=n, dt=0.01)
    x = field(n, 'prior')
    f64, f32 = flows(n, 0.01)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    y = chain.transition(xd)
    assert y.requires_grad
    check('torch route n=16 requires_grad', y, f32.transition(x), f64.transition(x))
    check('kernel route n=16', chain.transition(xd.detach()), f32.transition(x), f64.transition(x))
    with pytest.raises(_lib.SdaHipError):                              # a CPU tensor at a served size: as Lorenz63
        chain.transition(torch.from_numpy(x))


DRIVER = ('from sda.mcs import *\nfrom sda.score import *\nfrom sda.utils import *\n'
          'def make_chain() -> MarkovChain:\n    return KolmogorovFlow(size=32, dt=0.2)\n')
SCRIPT = '''import sys
sys.path.insert(0, {root!r})
import sda_amd
sda_amd.install_as_sda(native_chains=True)
sys.path.insert(0, 'experiments/kolmogorov')
from utils import *
chain = make_chain()
x = chain.prior((2,), device='cuda')
t = chain.trajectory(x, 4)
c = KolmogorovFlow.coarsen(t, 4)
assert torch.isfinite(t).all()
print('DROPIN', type(chain).__module__, chain.steps, tuple(x.shape), tuple(t.shape), tuple(c.shape))
'''


def test_dropin_driver_with_native_flow(dev, tmp_path):
    """A stand-in experiments/kolmogorov/utils.py (the reference's star imports; make_chain at size 32 for time) in a fresh child."""
    (tmp_path / 'experiments' / 'kolmogorov').mkdir(parents=True)
    (tmp_path / 'experiments' / 'kolmogorov' / 'utils.py').write_text(DRIVER)
    out = subprocess.run([sys.executable, '-B', '-c', SCRIPT.format(root=ROOT)], cwd=tmp_path, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('DROPIN')][0]
    assert line == f"DROPIN sda_amd.chains {R.steps_for(32, 0.2)} (2, 2, 32, 32) (4, 2, 2, 32, 32) (4, 2, 2, 8, 8)"


def test_generate_tool_writes_loadable_splits(dev, tmp_path):
    """tools/kolmogorov_generate.py at a small size: 10 trajectories in batches of 4, split 8 / 1 / 1, loadable as a dataset."""
    from sda_amd.data import DeviceTrajectories
    out = subprocess.run([sys.executable, '-B', os.path.join(ROOT, 'tools', 'kolmogorov_generate.py'), '--trajectories', '10', '--batch',
                          '4', '--size', '32', '--length', '6', '--keep', '4', '--out', str(tmp_path)], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    shapes = {k: np.load(tmp_path / f'{k}.npy').shape for k in ('train', 'valid', 'test')}
    assert shapes == {'train': (8, 4, 2, 8, 8), 'valid': (1, 4, 2, 8, 8), 'test': (1, 4, 2, 8, 8)}
    data = DeviceTrajectories(np.load(tmp_path / 'train.npy'), window=3, flatten=True, device=dev)
    assert data.data.shape == (8, 4, 2, 8, 8) and torch.isfinite(data.data).all()
