"""CPU: the Kolmogorov-flow chain without a device -- sub-step counts, the NumPy restatement's own invariants in float64
(tests/kflow_ref.py), the torch-ops route of ``sda_amd.chains.KolmogorovFlow`` against it, the install switch and the ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains
from tests import kflow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smooth_field(n, seed=0, batch=()):
    """A prior draw of the replay (float64): smooth, divergence-free, max speed 3."""
    z = np.random.default_rng(seed).standard_normal((*batch, 2, n, n))
    return R.Flow(n, 0.2).prior(z)


@pytest.mark.parametrize('size,dt', [(256, 0.2), (64, 0.2), (256, 0.01), (16, 0.5)])
def test_substep_counts(size, dt):
    chain = chains.KolmogorovFlow(size=size, dt=dt)
    assert chain.steps == R.steps_for(size, dt) == R.Flow(size, dt).steps
    if (size, dt) == (256, 0.2):
        assert chain.steps == 82
    assert chain.delta == float(np.float32(dt / chain.steps))


@pytest.mark.parametrize('n', [16, 48])
def test_replay_projection_is_exact_and_idempotent(n):
    f = R.Flow(n, 0.2)
    x = f.explicit(_smooth_field(n, 1))
    p = f.project(x)
    assert np.abs(f.divergence(p)).max() <= 1e-10 * np.abs(x).max() / f.h
    assert np.abs(f.project(p) - p).max() <= 1e-10 * np.abs(x).max()
    assert np.abs(f.divergence(x)).max() > 1e-6                      # the projection had something to remove


@pytest.mark.parametrize('n', [16, 48, 64])
def test_replay_laminar_state_is_a_fixed_point(n):
    f = R.Flow(n, 0.2)
    x, A = f.laminar()
    assert A > 1 and np.abs(f.substep(x) - x).max() <= 1e-12


@pytest.mark.parametrize('n', [16, 48])
def test_hartley_matrix_diagonalises_the_laplacian(n):
    H, L = R.hartley_matrix(n), R.laplacian_matrix(n)
    assert np.abs(H - H.T).max() == 0
    assert np.abs(H @ H - np.eye(n)).max() < 1e-13
    D = H @ L @ H
    assert np.abs(D - np.diag(R.eigenvalues(n))).max() < 1e-11 * np.abs(L).max()
    x = np.random.default_rng(2).standard_normal((n, n))
    assert np.abs(R.hartley2(x) - H @ x @ H).max() < 1e-12
    # an even radial filter is pointwise in the Hartley domain too
    g = R.prior_filter(n)
    assert np.abs(H @ (g * (H @ x @ H)) @ H - np.fft.ifft2(np.fft.fft2(x) * g).real).max() < 1e-12


@pytest.mark.parametrize('n', [16, 48])
@pytest.mark.parametrize('field', ['prior', 'ties'])
def test_torch_route_against_the_replay(n, field):
    """explicit terms and the full sub-step of the torch-ops route in float32 under the tolerance rule."""
    chain = chains.KolmogorovFlow(size=n, dt=0.2)
    f64, f32 = R.Flow(n, 0.2, dtype=np.float64), R.Flow(n, 0.2, dtype=np.float32)
    x = _smooth_field(n, 3).astype(np.float32) if field == 'prior' else R.ties_field(n)
    xt = torch.from_numpy(x)
    for name, got, r32, r64 in (('explicit', chain._torch_explicit(xt), f32.explicit(x), f64.explicit(x)),
                                ('substep', chain._torch_substep(xt), f32.substep(x), f64.substep(x))):
        b, own = R.bound(r32, r64)
        err = np.abs(got.numpy().astype(np.float64) - r64).max()
        print(f'torch {name} n={n} {field}: own {own:.3e} error {err:.3e} bound {b:.3e}')
        assert got.dtype == torch.float32 and err <= b, (name, err, b)


def test_torch_route_in_float64_and_its_gradient():
    """float64: the route equals the float64 replay to rounding, and its vector-Jacobian product agrees with central finite
    differences of one sub-step at N = 16."""
    n = 16
    chain = chains.KolmogorovFlow(size=n, dt=0.2)
    x = _smooth_field(n, 4)
    xt = torch.from_numpy(x).requires_grad_()
    y = chain._torch_substep(xt)
    assert np.abs(y.detach().numpy() - R.Flow(n, 0.2).substep(x)).max() <= 1e-12 * np.abs(x).max()
    rng = np.random.default_rng(5)
    w = torch.from_numpy(rng.standard_normal(x.shape))
    g, = torch.autograd.grad((y * w).sum(), xt)
    for _ in range(6):
        d = torch.from_numpy(rng.standard_normal(x.shape))
        eps = 1e-6
        with torch.no_grad():
            fd = ((chain._torch_substep(xt + eps * d) - chain._torch_substep(xt - eps * d)) * w).sum() / (2 * eps)
        an = (g * d).sum()
        assert abs(float(fd - an)) <= 1e-6 * max(1.0, abs(float(an))), (float(fd), float(an))
    # an input that requires grad takes this route through the public method, at a size the kernels serve
    out = chain.transition(xt)
    assert out.requires_grad and out.dtype == torch.float64


def test_torch_route_tables_are_built_once():
    """The torch-ops route reads its solve table and forcing profile every sub-step: they come from a per-(size, device, dtype)
    cache, equal the float64 tables rounded once, and a transition builds nothing on the host after its first sub-step."""
    from sda_amd import ops
    n = 20
    inv, forcing = ops.kflow_solve_tables(n, 'cpu', torch.float32)
    again = ops.kflow_solve_tables(n, torch.device('cpu'), torch.float32)
    assert again[0] is inv and again[1] is forcing
    hm, inv64, forcing64 = ops.kflow_tables(n)
    assert torch.equal(inv, inv64.float()) and torch.equal(forcing, forcing64.float()) and inv[0, 0] == 0
    assert ops.kflow_solve_tables(n, 'cpu', torch.float64)[0].dtype == torch.float64
    built = []
    real = ops._kflow_solve_tables
    ops._kflow_solve_tables = lambda m: built.append(m) or real(m)
    try:
        chain = chains.KolmogorovFlow(size=24, dt=0.2)
        assert chain.steps > 1
        chain.transition(torch.from_numpy(_smooth_field(24, 7).astype(np.float32)))
    finally:
        ops._kflow_solve_tables = real
    assert built == [24]


def test_unserved_size_and_cpu_tensor():
    chain = chains.KolmogorovFlow(size=20, dt=0.01)                   # 20 % 16 != 0: torch ops, also on the host
    x = torch.from_numpy(_smooth_field(20, 6).astype(np.float32))
    want = R.Flow(20, 0.01, dtype=np.float64).transition(x.numpy())
    b, own = R.bound(R.Flow(20, 0.01, dtype=np.float32).transition(x.numpy()), want)
    assert np.abs(chain.transition(x).numpy() - want).max() <= b
    assert chain.trajectory(x, 2).shape == (2, 2, 20, 20)
    served = chains.KolmogorovFlow(size=16, dt=0.01)
    with pytest.raises(_lib.SdaHipError):                             # as Lorenz63: the kernels have no CPU form
        served.transition(torch.zeros(2, 16, 16))
    with pytest.raises(_lib.SdaHipError):
        served.transition(torch.zeros(2, 32, 32))
    assert chains.KolmogorovFlow.coarsen(torch.ones(2, 8, 8), 4).shape == (2, 2, 2)
    assert chains.KolmogorovFlow.vorticity(torch.ones(2, 8, 8)).shape == (8, 8)
    assert chains.KolmogorovFlow.upsample(torch.ones(2, 4, 4), 2).shape == (2, 8, 8)


def test_make_chain():
    from sda_amd.experiments import kolmogorov
    chain = kolmogorov.make_chain()
    assert type(chain) is chains.KolmogorovFlow and (chain.size, chain.dt, chain.steps) == (256, 0.2, 82)


def test_install_rebinds_kolmogorov_flow():
    code = ('import sys\nsys.path.insert(0, %r)\nimport sda_amd\nsda_amd.install_as_sda(native_chains=%s)\n'
            'from sda.mcs import *\n'
            'try:\n'
            '    c = KolmogorovFlow(size=64, dt=0.2)\n'
            '    print("CHAIN", type(c).__module__, c.steps, KolmogorovFlow.coarsen(torch.ones(2, 8, 8), 4).shape[-1])\n'
            'except ImportError as e:\n'
            '    print("PLACEHOLDER", "rebuild" in str(e))\n')
    env = {k: v for k, v in os.environ.items() if k != 'SDA_MCS_FILE'}
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'True')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['CHAIN', 'sda_amd.chains', str(R.steps_for(64, 0.2)), '2']
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'False')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['PLACEHOLDER', 'True']


def test_abi_lists_the_kflow_entries(tmp_path):
    import ctypes
    from sda_amd import build
    header = open(os.path.join(ROOT, 'include', 'sda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = ['sda_kflow_serves', 'sda_kflow_work_floats', 'sda_kflow_explicit', 'sda_kflow_hartley', 'sda_kflow_project',
             'sda_kflow_advance']
    assert 'kflow.hip' in build.SOURCES
    build.build()
    lib = _lib.load()
    for n in names:
        assert re.search(r'\b%s\s*\(' % n, text) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('sda_kflow_')) == sorted(names)
    assert '#define SDA_ABI_VERSION 14' in header and lib.sda_abi_version() == 14
    fields = [f[0] for f in _lib.KflowModel._fields_]
    src = tmp_path / 'layout.c'
    prints = '\n'.join(f'printf("{f} %zu\\n", offsetof(sda_kflow_model, {f}));' for f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/sda_hip.h"\nint main(){{printf("size %zu\\n", '
                   f'sizeof(sda_kflow_model));\n{prints}\nreturn 0;}}')
    subprocess.check_call(['gcc', str(src), '-o', str(tmp_path / 'layout')])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / 'layout')]).decode().splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.KflowModel)
    for f in fields:
        assert int(got[f]) == getattr(_lib.KflowModel, f).offset, f
    # sizes and bad arguments are settled on the host, before any launch
    assert [lib.sda_kflow_serves(n) for n in (16, 48, 256, 272, 512, 8, 20, 528)] == [1, 1, 1, 1, 1, 0, 0, 0]
    assert lib.sda_kflow_work_floats(64, 3) == 6 * 3 * 64 * 64 and lib.sda_kflow_work_floats(20, 1) == 0
    assert lib.sda_kflow_advance(None, None, 0, 1, 1, 0, None, 0, None, None) == -1
    assert lib.sda_kflow_hartley(None, 16, None, 256, 1, 0, None, None, None) == -1
