"""GPU: the ensemble Kalman smoother kernels (csrc/enks.hip) against the float64 numpy replay (tests/enks_ref.py) under the project's
bound rule, against their host twins, their reproducibility, ``chains.enks_fused`` end to end with every analysis replayed from the
recorded ensemble, the convergence of ``spring.enks`` to the exact smoother, and ``lorenz.enks`` on the 'lo' protocol."""
import numpy as np
import pytest
import torch

from tests import enks_ref as R
from tests.chain_util import bound

pytestmark = pytest.mark.gpu

CASES = [(m, d, k, w, lam, sig) for (m, d, k) in R.SHAPES for w in R.WINDOWS for lam in R.INFLATIONS for sig in R.SIGMAS]
CASES.append((16384, 3, 1, R.WINDOWS[1], 1.05, 1.0))
GUARD = 12345.0


def _device_analysis(c, lo, t, sigma, inflation, *, extra=0):
    """The two ops on a time-strided view (every other slab, from slab 1) of a larger tensor: (view, big, a, z, status)."""
    from sda_amd import ops
    S0 = c['S']
    slabs, m, d = S0.shape
    big = torch.full((2 * (slabs + extra) + 1, m, d), GUARD, device='cuda')
    S = big[1::2]
    S[:slabs] = torch.from_numpy(S0.copy()).cuda()
    index, shift, scale = c['obs']
    o = ops.chain_obs(index, shift, scale, sigma, torch.from_numpy(c['y'].copy()).cuda())
    a, z, status = ops.enks_gain(S, t, o, inflation=inflation, seed=c['seed'], draw=c['draw'])
    ops.enks_update(S, lo, t, a, z, inflation=inflation)
    return S, big, a, z, status


def _check(c, lo, t, S, a, z):
    (S64, a64, z64), (S32, a32, z32) = c['ref64'], c['ref32']
    for name, got, r32, r64 in (('a', a, a32, a64), ('z', z, z32, z64), ('S', S[lo:t + 1], S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got.double().cpu().numpy() - r64).max(), bound(r32, r64)
        print(f'{name}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize('m,d,k,window,inflation,sigma', CASES)
def test_ops_match_the_float64_replay(m, d, k, window, inflation, sigma):
    slabs, lo, t = window
    c = R.case(m, d, k, slabs, lo, t, inflation, sigma)
    S, big, a, z, status = _device_analysis(c, lo, t, sigma, inflation)
    assert int(status) == 0
    _check(c, lo, t, S[:slabs], a, z)
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(torch.equal(S[s].cpu(), torch.from_numpy(c['S'][s].copy())) for s in outside)      # bitwise untouched
    assert bool((big[0::2] == GUARD).all())                                                             # and so is what lies between


@pytest.mark.parametrize('m,d,k', [(67, 3, 1), (1000, 5, 3), (130, 64, 64)])
def test_device_matches_the_host_twin(m, d, k):
    slabs, lo, t = R.WINDOWS[2]
    c = R.case(m, d, k, slabs, lo, t, 1.05, 1.0)
    index, shift, scale = c['obs']
    Sh, ah, zh, status, rcs = R.host_analysis(c['S'], lo, t, index, shift, scale, 1.0, c['y'], c['seed'], c['draw'], 1.05)
    assert rcs == (0, 0) and status == 0
    S, _, a, z, _ = _device_analysis(c, lo, t, 1.0, 1.05)
    (S64, a64, z64), (S32, a32, z32) = c['ref64'], c['ref32']
    for name, got, host, r32, r64 in (('a', a, ah, a32, a64), ('z', z, zh, z32, z64), ('S', S[:slabs], Sh, S32, S64)):
        err, tol = np.abs(got.double().cpu().numpy() - host.astype(np.float64)).max(), bound(r32, r64)
        print(f'{name}: device - host {err:.3e} bound {tol:.3e}')
        assert err <= tol, (name, err, tol)


def test_reproducible_and_independent_of_unrelated_slabs():
    slabs, lo, t = R.WINDOWS[2]
    c = R.case(256, 40, 20, slabs, lo, t, 1.05, 1.0)
    first = _device_analysis(c, lo, t, 1.0, 1.05)
    again = _device_analysis(c, lo, t, 1.0, 1.05)
    longer = _device_analysis(c, lo, t, 1.0, 1.05, extra=5)
    for other in (again, longer):
        assert torch.equal(first[0][:slabs], other[0][:slabs]) and torch.equal(first[2], other[2]) and torch.equal(first[3], other[3])
    assert bool((longer[0][slabs:] == GUARD).all())


def _pairs():
    from sda_amd import chains
    l63 = chains.NoisyLorenz63(dt=0.025)
    yield 'l63', l63, chains.probe_affine(lambda x: l63.preprocess(x)[..., :1], l63, 3), None, 1.0
    yield 'l96', chains.Lorenz96(n=8), chains.AffineObservation(range(0, 8, 2), [0.0] * 4, [1.0] * 4), 2, 1.05


@pytest.mark.parametrize('name', ['l63', 'l96'])
def test_enks_fused_replays_analysis_by_analysis(name):
    from sda_amd import chains
    _, chain, obs, lag, inflation = next(p for p in _pairs() if p[0] == name)
    assert obs is not None
    torch.manual_seed(3)
    m, n, step, sigma = 256, 4, 2, 0.5
    x = chain.trajectory(chain.prior((m,), device='cuda'), 16, last=True)
    truth = chain.trajectory(x[:1], n * step)[step - 1::step, 0]
    y = obs(truth) + sigma * torch.randn(n, len(obs.index), device='cuda')
    draw_before = chain._draw
    record = {}
    out = chains.enks_fused(chain, x, y, obs, sigma, step, lag=lag, inflation=inflation, seed=99, record=record)
    assert out.shape == (m, n * step + 1, x.shape[1]) and bool(torch.isfinite(out).all())
    assert chain._draw == draw_before + n * step
    assert record['status'].tolist() == [0] * n
    after = record['S'][1:] + [out.permute(1, 0, 2)]
    for i in range(n):
        t = (i + 1) * step
        lo = 0 if lag is None else max(0, t - lag * step)
        pre = record['S'][i].cpu().numpy()[:t + 1]
        args = (pre, lo, t, obs.index, obs.shift, obs.scale, sigma, y[i].cpu().numpy(), R.perturbations(m, len(obs.index), 99, i), inflation)
        (S64, a64, z64), (S32, a32, z32) = R.analysis(*args, np.float64), R.analysis(*args, np.float32)
        got = after[i][:t + 1]
        for nm, g, r32, r64 in (('a', record['a'][i], a32, a64), ('z', record['z'][i], z32, z64), ('S', got, S32, S64)):
            err, tol = np.abs(g.double().cpu().numpy() - r64).max(), bound(r32, r64)
            print(f'analysis {i} {nm}: err {err:.3e} bound {tol:.3e}')
            assert err <= tol, (i, nm, err, tol)
        assert torch.equal(after[i][:lo].cpu(), record['S'][i][:lo].cpu())          # before the window: untouched


def test_spring_enks_converges_to_the_exact_smoother():
    """Both error measures at least halve from M = 1024 to M = 16 384, the RMS taken over all (time, component) entries of FOUR
    seeded runs per size.  One run per size is too noisy a statistic: the members share one estimated gain, so a run's errors
    are correlated and its RMS is close to a single draw.  With seed 0 alone the device gives 0.0413 -> 0.0242 (ratio 0.59) for the
    mean and 0.0418 -> 0.0061 (0.15) for the variance, and a float64 numpy replay of exactly that run's random inputs gives the
    same four figures to six digits (profiles/enks_parity.txt), so that ratio is the realisation, not the arithmetic.  Pooled over
    seeds 0 .. 3 the float64 replay of the same inputs gives ratios 0.33 and 0.19."""
    from sda_amd.experiments import spring
    sigma, step, n_obs, burn = 0.1, 4, 8, 64
    y = torch.from_numpy(R.spring_observations(n_obs, step, sigma, burn, 0))
    A = lambda x: x[..., :1]  # noqa: E731
    mean, cov, _ = spring.posterior_moments(y, A, sigma, step, burn=burn)
    errs = {1024: [], 16384: []}
    torch.manual_seed(0)
    for seed in range(4):
        for members in (1024, 16384):
            x = spring.enks(y, A, sigma, step, members, burn=burn, seed=seed, device='cuda')
            assert x.shape == (members, (n_obs - 1) * step + 1, 4)
            errs[members].append(R.moment_errors(x.double().cpu().numpy(), mean.numpy(), cov.numpy()))
            print(f'seed {seed} M = {members}: RMS mean error / exact std {errs[members][-1][0]:.4f}, RMS relative variance error '
                  f'{errs[members][-1][1]:.4f}')
    pooled = {m: [float(np.sqrt(np.mean([e[i] ** 2 for e in errs[m]]))) for i in (0, 1)] for m in errs}
    print(f'pooled: {pooled}')
    assert pooled[16384][0] < 0.5 * pooled[1024][0], pooled
    assert pooled[16384][1] < 0.5 * pooled[1024][1], pooled


def test_lorenz_enks_on_the_lo_protocol():
    from sda_amd._lib import SdaHipError
    from sda_amd.experiments import lorenz
    torch.manual_seed(1)
    sigma, step, n_obs, members = 0.05, 8, 9, 1024
    chain = lorenz.make_chain()
    A = lambda x: chain.preprocess(x)[..., :1]  # noqa: E731
    x = chain.trajectory(chain.prior((1,), device='cuda'), 64, last=True)
    truth = chain.trajectory(x, n_obs * step)[step - 1::step, 0]
    y = A(truth) + sigma * torch.randn(n_obs, 1, device='cuda')
    out = lorenz.enks(y, A, sigma, step, members, seed=5)
    assert out.shape == lorenz.posterior(y, A, sigma, step, seed=5)[:members].shape
    assert bool(torch.isfinite(out).all())
    free = lorenz.make_chain()
    x0 = free.trajectory(free.prior((members,), device='cuda'), 64, last=True)
    forecast = free.trajectory(x0, n_obs * step).mean(dim=1)[step - 1:]
    ll_enks = lorenz.log_likelihood(y, out.mean(dim=0), A, sigma, step)
    ll_free = lorenz.log_likelihood(y, forecast, A, sigma, step)
    print(f'log-likelihood of the mean trajectory: enks {float(ll_enks):.2f}, unconditioned forecast {float(ll_free):.2f}')
    assert float(ll_enks) > float(ll_free)
    with pytest.raises(SdaHipError):
        lorenz.enks(y, lambda x: x[..., :1] ** 2, sigma, step, members)
