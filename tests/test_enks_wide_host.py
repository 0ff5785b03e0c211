"""CPU: the ensemble-space smoother (csrc/enks_wide.hip).  The float64 replay of tests/enks_wide_ref.py against the observation-space
replay of tests/enks_ref.py; that no case's bound is vacuous; the host twins against the replay under the project's bound rule;
their refusals; the unchanged ABI; a non-finite observation; and the routes of ``lorenz.enks`` / ``spring.enks``."""
import ctypes

import numpy as np
import pytest
import torch

from tests import enks_ref
from tests import enks_wide_ref as R
from tests import observe_ref
from tests.chain_util import bound

IDS = [f'M{m}-d{d}-k{k}-{name}-w{w[0]}-lam{lam}-sig{sig}' for (m, d, k, name, w, lam, sig) in R.CASES]


@pytest.mark.parametrize('m,d,k,name,window,inflation,sigma', R.CASES, ids=IDS)
def test_the_bound_of_a_case_is_not_vacuous(m, d, k, name, window, inflation, sigma):
    """The fp32 replay must itself be close: a bound above 1e-4 of max|ref64| would let almost anything pass."""
    slabs, lo, t = window
    c = R.case(m, d, k, name, slabs, lo, t, inflation, sigma)
    S64, S32 = c['ref64'][0], c['ref32'][0]
    tol = bound(S32[lo:t + 1], S64[lo:t + 1])
    print(f'bound {tol:.3e} of max {np.abs(S64).max():.3e}')
    assert tol < 1e-4 * np.abs(S64).max()


SHARED = [(i, c) for i, c in zip(IDS, R.CASES) if R.shared(*c[:4])]


@pytest.mark.parametrize('m,d,k,name,window,inflation,sigma', [c for _, c in SHARED], ids=[i for i, _ in SHARED])
def test_float64_replay_agrees_with_the_observation_space_replay(m, d, k, name, window, inflation, sigma):
    """1e-9 of max|S| between the two float64 forms on every shared case: the shapes both smoothers serve (d <= 64, k <= 64), see
    ``enks_wide_ref.shared`` for why the observation-space replay is no yardstick at that tolerance beyond them."""
    slabs, lo, t = window
    c = R.case(m, d, k, name, slabs, lo, t, inflation, sigma)
    index, shift, scale = R.selection(d, k)
    S64 = enks_ref.analysis(c['S'], lo, t, index, shift, scale, sigma, c['y'], c['eps'], inflation, np.float64)[0]
    err = np.abs(S64 - c['ref64'][0]).max()
    print(f'ensemble space - observation space {err:.3e}')
    assert err <= 1e-9 * np.abs(c['S']).max()


def test_the_numpy_operator_is_the_reference_operator():
    x = np.random.default_rng(0).standard_normal((3, 512))
    A = observe_ref.Chain((3, 2, 16, 16), observe_ref.vorticity, lambda s: observe_ref.coarsen(s, 2))
    assert np.abs(R.operator('vortcoarse', 512, 64)(x, np.float64) - A.forward(x.reshape(3, 2, 16, 16)).reshape(3, 64)).max() < 1e-14
    P = observe_ref.Pointwise((3, 512), 'saturate')
    assert np.array_equal(R.operator('saturate', 512, 512)(x, np.float64), P.forward(x))


@pytest.mark.parametrize('m,d,k,name,window,inflation,sigma', R.CASES, ids=IDS)
def test_host_twins_match_the_float64_replay(m, d, k, name, window, inflation, sigma):
    slabs, lo, t = window
    c = R.case(m, d, k, name, slabs, lo, t, inflation, sigma)
    S, H, w = R.host_analysis(c, lo, t, sigma, inflation)
    assert w['rcs'] == (0, 0, 0) and int(w['status'][0]) == 0
    (S64, H64, W64), (S32, H32, W32) = c['ref64'], c['ref32']
    for nm, got, r32, r64 in (('H', H, H32, H64), ('S', S[lo:t + 1], S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got.astype(np.float64) - r64).max(), bound(r32, r64)
        print(f'{nm}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (nm, err, tol)
    # the stream of enks_fused: the same Philox words; logf / sincosf of two libms differ by an ulp or two of values below 8
    assert np.abs(w['eps'] - c['eps']).max() <= 4 * 2.0 ** -21
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(np.array_equal(S[s], c['S'][s]) for s in outside)        # bitwise untouched


def test_gram_partials_are_the_chunked_products():
    c = R.case(67, 512, 517, 'select', 3, 1, 1, 1.0, 1.0)
    w = R.host_weights(c['ref32'][1], c['y'], 1.0, c['seed'], c['draw'])
    part = w['part'].reshape(2, 80, 160)
    Y, D = w['Y'].astype(np.float64), w['D'].astype(np.float64)
    for ch, sl in enumerate((slice(0, R.KC), slice(R.KC, 517))):
        np.testing.assert_allclose(part[ch, :67, :67], Y[:, sl] @ Y[:, sl].T, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(part[ch, :67, 80:147], Y[:, sl] @ D[:, sl].T, rtol=1e-12, atol=1e-12)
    assert not part[:, 67:].any() and not part[:, :, 67:80].any() and not part[:, :, 147:].any()


def test_an_infinite_observation_sets_the_status_and_leaves_the_window_untouched():
    c = R.case(15, 48, 5, 'select', 4, 1, 2, 1.0, 1.0)
    y = np.array(c['y'])
    y[2] = np.inf
    S, H, w = R.host_analysis(c, 1, 2, 1.0, 1.0, y=y)
    assert w['rcs'] == (0, 0, 0) and int(w['status'][0]) == 1 and not w['W'].any()
    assert np.array_equal(S, c['S'])


def test_unit_inflation_touches_nothing():
    c = R.case(15, 48, 5, 'select', 4, 1, 2, 1.0, 1.0)
    S = np.array(c['S'])
    assert R.host_inflate(S, 2, 1.0) == 0 and np.array_equal(S, c['S'])
    assert R.host_inflate(S, 2, 1.05) == 0 and not np.array_equal(S[2], c['S'][2]) and np.array_equal(S[:2], c['S'][:2])


def _entries(lib, host):
    sfx, tail = ('_host', ()) if host else ('', (None,))
    P = 0x10000
    return {
        'prepare': lambda m, k, **kw: getattr(lib, 'sda_enkw_prepare' + sfx)(
            kw.get('H', P), m, k, P, kw.get('sigma', 1.0), 0, kw.get('draw', 0), P, P, None, *((None,) if host else ()), *tail),
        'gram': lambda m, k, **kw: getattr(lib, 'sda_enkw_gram' + sfx)(kw.get('H', P), P, m, k, P, *tail),
        'solve': lambda m, k, **kw: getattr(lib, 'sda_enkw_solve' + sfx)(kw.get('H', P), m, k, kw.get('sigma', 1.0), P, P, P, *tail),
    }


@pytest.mark.parametrize('host', [True, False], ids=['host-twins', 'device-entries'])
def test_refusals_before_anything_runs(host):
    """Every entry refuses on the host, before a launch or a memory access: the pointers here are not mapped."""
    from sda_amd import _lib
    lib = R.emu() if host else _lib.load()
    P = 0x10000
    e = _entries(lib, host)
    for name, fn in e.items():
        assert fn(129, 4) == -2 and fn(1, 4) == -2, name              # SDA_E_UNSUPPORTED
        assert fn(0, 4) == -1 and fn(8, 0) == -1 and fn(8, 4, H=None) == -1, name
    assert e['prepare'](8, 4, sigma=0.0) == -1 and e['prepare'](8, 4, draw=-1) == -1 and e['solve'](8, 4, sigma=-1.0) == -1
    tr = getattr(lib, 'sda_enkw_transform' + ('_host' if host else ''))
    tail = () if host else (None,)
    assert tr(P, 8 * 4, 4, 1, 129, 4, P, 1.0, 0, *tail) == -2 and tr(P, 4, 4, 1, 1, 4, P, 1.0, 0, *tail) == -2
    assert tr(P, 32, 4, 65536, 8, 4, P, 1.0, 0, *tail) == -2
    for bad in ((None, 32, 4, 1, 8, 4, P, 1.0, 0), (P, 32, 3, 1, 8, 4, P, 1.0, 0), (P, 32, 4, 0, 8, 4, P, 1.0, 0),
                (P, 32, 4, 1, 8, 0, P, 1.0, 0), (P, 32, 4, 1, 8, 4, None, 1.0, 0), (P, 32, 4, 1, 8, 4, P, 0.0, 1),
                (P, 32, 4, 1, 8, 4, P, 1.0, 2), (P, -1, 4, 1, 8, 4, P, 1.0, 0)):
        assert tr(*bad, *tail) == -1, bad
    assert lib.sda_enkw_gram_doubles(129, 4) == 0 and lib.sda_enkw_gram_doubles(67, 517) == 2 * 80 * 160


def test_abi_14_is_unchanged_and_the_new_symbols_resolve():
    from sda_amd import _lib
    lib = _lib.load()
    assert lib.sda_abi_version() == 14
    names = ['sda_enkw_gram_doubles', 'sda_enkw_prepare', 'sda_enkw_gram', 'sda_enkw_solve', 'sda_enkw_transform']
    assert all(n in _lib.SIGNATURES and getattr(lib, n) is not None for n in names)
    assert 'sda_enks_gain' in _lib.SIGNATURES and 'sda_enks_update' in _lib.SIGNATURES
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.__file__)), 'include', 'sda_hip.h')) as f:
        header = f.read()
    assert all(f' {n}(' in header for n in names)


def test_ops_check_their_arguments_without_a_device():
    from sda_amd import ops
    from sda_amd._lib import SdaHipError
    with pytest.raises(SdaHipError):
        ops.enkw_prepare(torch.zeros(4, 3), torch.zeros(3), 1.0)          # CPU tensors: no fallback
    with pytest.raises(SdaHipError):
        ops.enkw_gram(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(SdaHipError):
        ops.enkw_transform(torch.zeros(2, 4, 3), 0, 1, torch.zeros(4, 4))
    with pytest.raises(SdaHipError):
        ops.enkw_inflate(torch.zeros(2, 4, 3), 0, 1.05)


@pytest.mark.parametrize('module', ['lorenz', 'spring'])
def test_the_two_routes_of_a_smoother(module, monkeypatch):
    """space='observation' (the default) calls ``chains.enks_fused`` with the probed selection, as before; space='ensemble' calls
    ``chains.enks_wide`` with A itself and probes nothing."""
    import importlib
    from sda_amd import chains
    exp = importlib.import_module(f'sda_amd.experiments.{module}')
    calls = []

    class Chain:
        d = 4

        def prior(self, shape, device=None):
            return torch.zeros(*shape, 4)

        def trajectory(self, x, length, last=False, **kw):
            return x

    def fused(chain, x, y, obs, sigma, step, **kw):
        calls.append(('fused', obs, kw))
        return torch.zeros(x.shape[0], len(y) * step + 1, 4)

    def wide(chain, x, y, A, sigma, step, **kw):
        calls.append(('wide', A, kw))
        return torch.zeros(x.shape[0], len(y) * step + 1, 4)

    def probe(A, chain, d):
        calls.append(('probe', A, d))
        return 'selection'

    monkeypatch.setattr(chains, 'enks_fused', fused)
    monkeypatch.setattr(chains, 'enks_wide', wide)
    monkeypatch.setattr(chains, 'probe_affine', probe)
    A = lambda x: x[..., :1] ** 2  # noqa: E731
    y = torch.zeros(3, 1)
    out = exp.enks(y, A, 0.5, 2, 8, chain=Chain(), burn=0, seed=1, device='cpu', lag=1, inflation=1.05)
    assert [c[0] for c in calls] == ['probe', 'fused'] and calls[1][1] == 'selection'
    assert calls[1][2] == dict(lag=1, inflation=1.05, seed=1) and out.shape == (8, 5, 4)
    del calls[:]
    out = exp.enks(y, A, 0.5, 2, 8, chain=Chain(), burn=0, seed=1, device='cpu', lag=1, inflation=1.05, space='ensemble')
    assert [c[0] for c in calls] == ['wide'] and calls[0][1] is A
    assert calls[0][2] == dict(lag=1, inflation=1.05, seed=1) and out.shape == (8, 5, 4)
    with pytest.raises(ValueError):
        exp.enks(y, A, 0.5, 2, 8, chain=Chain(), space='k')
