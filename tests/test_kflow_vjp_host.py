"""CPU: the adjoint of the Kolmogorov-flow sub-step without a device -- the gather-form restatement of the explicit terms' VJP
(tests/kflow_vjp_ref.py, written as the kernel is) against torch float64 autograd of the torch-ops route, the projection as its own
transpose, the new C entries and the opt-in switch."""
import os
import re

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains
from tests import kflow_ref as R
from tests import kflow_vjp_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', ['prior', 'ties'])
@pytest.mark.parametrize('n', [16, 20, 48])
def test_gather_form_against_autograd(n, kind):
    """float64: both sides evaluate the same piecewise-smooth branch, so they agree to rounding (1e-12 relative) -- on the ties
    field too, whose exact a == 0, d == 0 and r == 0 faces are where a wrong convention shows.  float32: under the tolerance rule."""
    chain = V.chain_for(n)
    x = V.prior_field(n, n) if kind == 'prior' else R.ties_field(n)
    if kind == 'ties':
        u, v = x.astype(np.float64)
        d = np.roll(u, -1, 0) - u
        assert (d == 0).any() and (0.5 * (v + np.roll(v, -1, 0)) == 0).any() and ((u - np.roll(u, 1, 0))[d != 0] == 0).any()
    g = V.cotangent(x.shape, 7)
    r32, r64 = V.oracles(chain._torch_explicit, x, g)
    got = V.explicit_vjp(R.Flow(n, 0.2), x, g)
    assert got.dtype == np.float64 and np.abs(got - r64).max() <= 1e-12 * np.abs(r64).max()
    b, own = V.bound_and_own(r32, r64)
    got32 = V.explicit_vjp(R.Flow(n, 0.2, dtype=np.float32), x, g)
    err = np.abs(got32.astype(np.float64) - r64).max()
    print(f'host vjp n={n} {kind}: own {own:.3e} error {err:.3e} bound {b:.3e}')
    assert got32.dtype == np.float32 and err <= b


def test_gather_form_takes_batches():
    n = 16
    x = V.prior_field(n, 3, (2,))
    g = V.cotangent(x.shape, 4)
    f = R.Flow(n, 0.2)
    both = V.explicit_vjp(f, x, g)
    assert both.shape == x.shape and np.array_equal(both[1], V.explicit_vjp(f, x[1], g[1]))


@pytest.mark.parametrize('n', [16, 20])
def test_projection_is_its_own_transpose(n):
    """<P a, b> = <a, P b> in float64: G = -D^T and the solve is symmetric, so the forward launches are the adjoint's too."""
    chain = V.chain_for(n)
    rng = np.random.default_rng(n)
    a, b = (torch.from_numpy(rng.standard_normal((2, n, n))) for _ in range(2))
    lhs, rhs = float((chain._torch_project(a) * b).sum()), float((a * chain._torch_project(b)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)) and abs(lhs) > 1e-3
    # and autograd agrees: the VJP of the projection is the projection of the cotangent
    vjp = V.autograd_vjp(chain._torch_project, a.numpy(), b.numpy(), torch.float64)
    assert np.abs(vjp - chain._torch_project(b).numpy()).max() <= 1e-12 * float(b.abs().max())


def test_grad_option_and_route_record():
    with pytest.raises(ValueError):
        chains.KolmogorovFlow(size=16, dt=0.2, grad='nonsense')
    assert chains.KolmogorovFlow(size=16, dt=0.2).grad == 'torch'
    from sda_amd.experiments import kolmogorov
    assert kolmogorov.make_chain().grad == 'torch' and kolmogorov.make_chain(grad='device').grad == 'device'
    # an unserved size keeps the torch route under either setting, on the host too
    chain = chains.KolmogorovFlow(size=20, dt=0.01, grad='device')
    x = torch.from_numpy(V.prior_field(20, 6))
    chain.transition(x)
    assert chains.LAST_KFLOW_GRAD_ROUTE is None
    y = chain.transition(x.clone().requires_grad_())
    assert y.requires_grad and chains.LAST_KFLOW_GRAD_ROUTE == 'torch'
    with torch.no_grad():
        chain.transition(x.clone().requires_grad_())
    assert chains.LAST_KFLOW_GRAD_ROUTE is None


def test_abi_lists_the_adjoint_entries():
    from sda_amd import build
    header = open(os.path.join(ROOT, 'include', 'sda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    build.build()
    lib = _lib.load()
    for name in ('sda_kfvjp_work_floats', 'sda_kfvjp_explicit', 'sda_kfvjp_transition'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert '#define SDA_ABI_VERSION 14' in header and lib.sda_abi_version() == 14
    # sizes and bad arguments are settled on the host, before any launch
    assert lib.sda_kfvjp_work_floats(64, 3, 11) == 13 * 2 * 3 * 64 * 64
    assert lib.sda_kfvjp_work_floats(20, 1, 1) == 0 and lib.sda_kfvjp_work_floats(64, 1, 0) == 0
    assert lib.sda_kfvjp_explicit(None, None, 0, None, 0, 1, None, None) == -1
    assert lib.sda_kfvjp_transition(None, None, 0, None, 0, 1, None, None, None) == -1
