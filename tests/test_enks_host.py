"""CPU: the host twins of the ensemble Kalman smoother (csrc/enks.hip under SDA_HOST_EMU) against the float64 numpy replay of the
five steps (tests/enks_ref.py) under the project's bound rule, their refusals, and the convergence of the algorithm itself to the
exact smoother of the damped spring as the ensemble grows.

Convergence figures of this set-up (float64 replay, component 0 observed, sigma 0.1, step 4, N 8, burn 64, seed 0), recorded in
profiles/enks_parity.txt: RMS mean error / exact std 0.0286 at M = 1024 and 0.0105 at M = 16 384 (ratio 0.37); RMS relative
variance error 0.0338 and 0.0070 (ratio 0.21)."""
import numpy as np
import pytest
import torch

from tests import enks_ref as R
from tests.chain_util import bound

CASES = [(m, d, k, w, lam, sig) for (m, d, k) in R.SHAPES for w in R.WINDOWS for lam in R.INFLATIONS for sig in R.SIGMAS]


@pytest.mark.parametrize('m,d,k,window,inflation,sigma', CASES)
def test_host_twins_match_the_float64_replay(m, d, k, window, inflation, sigma):
    slabs, lo, t = window
    c = R.case(m, d, k, slabs, lo, t, inflation, sigma)
    index, shift, scale = c['obs']
    S, a, z, status, rcs = R.host_analysis(c['S'], lo, t, index, shift, scale, sigma, c['y'], c['seed'], c['draw'], inflation)
    assert rcs == (0, 0) and status == 0
    (S64, a64, z64), (S32, a32, z32) = c['ref64'], c['ref32']
    for name, got, r32, r64 in (('a', a, a32, a64), ('z', z, z32, z64), ('S', S[lo:t + 1], S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got.astype(np.float64) - r64).max(), bound(r32, r64)
        print(f'{name}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (name, err, tol)
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(np.array_equal(S[s], c['S'][s]) for s in outside)        # bitwise untouched


def test_unit_inflation_leaves_the_observed_slab_to_the_update_alone():
    """lambda == 1: z == 0 (a failed factor is the one way to get it) must leave every slab bitwise as it was, the observed one
    included -- the inflation formula is not evaluated at all."""
    c = R.case(67, 3, 1, 4, 1, 2, 1.0, 1.0)
    lib = R.emu()
    S = np.array(c['S'])
    a = np.ascontiguousarray(c['ref32'][1], np.float32)
    z = np.zeros_like(a)
    assert lib.sda_enks_update_host(S[1].ctypes.data, 67 * 3, 3, 2, 67, 3, 1, 1.0, a.ctypes.data, z.ctypes.data) == 0
    assert np.array_equal(S, c['S'])


def test_a_failed_factorisation_sets_the_status_and_adds_nothing():
    c = R.case(67, 3, 1, 4, 1, 2, 1.0, 1.0)
    S = np.array(c['S'])
    S[2, 0, 2] = np.nan                                               # the observed component of one member
    index, shift, scale = c['obs']
    _, a, z, status, rcs = R.host_analysis(S, 1, 2, index, shift, scale, 1.0, c['y'], 0, 0, 1.0)
    assert rcs == (0, 0) and status == 1 and not z.any()


@pytest.mark.parametrize('m,d,index', [(1, 3, [0]), (8, 3, []), (8, 3, [0, 1, 2, 0]), (8, 65, [0])],
                         ids=['M=1', 'k=0', 'k>d', 'd=65'])
def test_refusals(m, d, index):
    k = len(index)
    S = np.ones((2, m, d), np.float32)
    before = S.copy()
    S2, a, z, status, (rc1, rc2) = R.host_analysis(S, 0, 1, index, [0.0] * k, [1.0] * k, 1.0, np.zeros(max(k, 1), np.float32), 0, 0, 1.0)
    assert rc1 in (-1, -2) and rc2 is None
    assert status == -1 and np.isnan(a).all() and np.isnan(z).all() and np.array_equal(S2, before)      # nothing was written
    a1 = np.zeros((max(k, 1), m), np.float32)
    rc = R.emu().sda_enks_update_host(S.ctypes.data, m * d, d, 2, m, d, k, 1.0, a1.ctypes.data, a1.ctypes.data)
    assert rc in (-1, -2) and np.array_equal(S, before)


def test_device_entries_refuse_the_same_shapes_before_any_launch():
    """The product library's entries run the same checks on the host: refused without touching a GPU."""
    import ctypes
    from sda_amd import _lib
    lib = _lib.load()
    P = 0x10000
    y = np.zeros(4, np.float32)
    for m, d, index in ((1, 3, [0]), (8, 3, []), (8, 3, [0, 1, 2, 0]), (8, 65, [0])):
        k = len(index)
        o = R.host_obs(index, [0.0] * k, [1.0] * k, 1.0, y)
        assert lib.sda_enks_gain(P, m, d, d, ctypes.byref(o), 1.0, 0, 0, P, P, P, P, None) in (-1, -2)
        assert lib.sda_enks_update(P, m * d, d, 1, m, d, k, 1.0, P, P, None) in (-1, -2)
    o = R.host_obs([0], [0.0], [1.0], 1.0, y)
    assert lib.sda_enks_gain(None, 8, 3, 3, ctypes.byref(o), 1.0, 0, 0, P, P, P, P, None) == -1
    assert lib.sda_enks_gain(P, 8, 3, 3, ctypes.byref(o), 0.0, 0, 0, P, P, P, P, None) == -1          # inflation <= 0
    assert lib.sda_enks_update(None, 24, 3, 1, 8, 3, 1, 1.0, P, P, None) == -1


def test_replay_converges_to_the_exact_smoother_of_the_damped_spring():
    """What catches a wrong algorithm rather than a wrong rounding: both error measures must at least halve from M = 1024 to
    M = 16 384 (the expected factor is sqrt(1024 / 16384) = 1 / 4)."""
    from sda_amd.experiments import spring
    sigma, step, n_obs, burn, seed = 0.1, 4, 8, 64, 0
    y = R.spring_observations(n_obs, step, sigma, burn, seed)
    mean, cov, _ = spring.posterior_moments(torch.from_numpy(y), lambda x: x[..., :1], sigma, step, burn=burn)
    mean, cov = mean.numpy(), cov.numpy()
    errs = {}
    for members in (1024, 16384):
        x = R.spring_enks(y, members, step, sigma, burn, seed)
        assert x.shape == (members, (n_obs - 1) * step + 1, 4)
        errs[members] = R.moment_errors(x, mean, cov)
        print(f'M = {members}: RMS mean error / exact std {errs[members][0]:.4f}, RMS relative variance error {errs[members][1]:.4f}')
    assert errs[16384][0] < 0.5 * errs[1024][0], errs
    assert errs[16384][1] < 0.5 * errs[1024][1], errs
