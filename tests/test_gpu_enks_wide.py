"""GPU: the ensemble-space smoother kernels (csrc/enks_wide.hip) against the float64 numpy replay (tests/enks_wide_ref.py) under the
project's bound rule, bitwise against their host twins, their reproducibility and slab independence, ``chains.enks_wide`` beside
``chains.enks_fused``, on the Kolmogorov flow with every analysis replayed, and the three experiment entries."""
import numpy as np
import pytest
import torch

from tests import enks_ref
from tests import enks_wide_ref as R
from tests.chain_util import bound

pytestmark = pytest.mark.gpu

IDS = [f'M{m}-d{d}-k{k}-{name}-w{w[0]}-lam{lam}-sig{sig}' for (m, d, k, name, w, lam, sig) in R.CASES]
GUARD = 12345.0


def _device_analysis(c, name, lo, t, sigma, inflation, *, extra=0, pad=3, y=None):
    """The ops on a time-strided, member-padded view of a larger tensor: dict(S, big, H, Y, D, eps, part, W, status)."""
    from sda_amd import ops
    S0 = c['S']
    slabs, m, d = S0.shape
    big = torch.full((2 * (slabs + extra) + 1, m, d + pad), GUARD, device='cuda')
    S = big[1::2, :, :d]
    S[:slabs] = torch.from_numpy(S0.copy()).cuda()
    ops.enkw_inflate(S, t, inflation)
    k = c['y'].shape[0]
    H = R.device_operator(name, d, k)(S[t].contiguous()).reshape(m, k).contiguous()
    yd = torch.from_numpy(np.array(c['y'] if y is None else y)).cuda()
    Y, D, eps = ops.enkw_prepare(H, yd, sigma, seed=c['seed'], draw=c['draw'])
    part = ops.enkw_gram(Y, D)
    W, status = ops.enkw_solve(part, m, k, sigma)
    ops.enkw_transform(S, lo, t, W)
    return dict(S=S, big=big, H=H, Y=Y, D=D, eps=eps, part=part, W=W, status=status)


@pytest.mark.parametrize('m,d,k,name,window,inflation,sigma', R.CASES, ids=IDS)
def test_ops_match_the_float64_replay(m, d, k, name, window, inflation, sigma):
    slabs, lo, t = window
    c = R.case(m, d, k, name, slabs, lo, t, inflation, sigma)
    r = _device_analysis(c, name, lo, t, sigma, inflation)
    assert int(r['status']) == 0
    (S64, H64, W64), (S32, H32, W32) = c['ref64'], c['ref32']
    S = r['S'][:slabs]
    for nm, got, r32, r64 in (('H', r['H'], H32, H64), ('S', S[lo:t + 1], S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got.double().cpu().numpy() - r64).max(), bound(r32, r64)
        print(f'{nm}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (nm, err, tol)
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(torch.equal(S[s].cpu(), torch.from_numpy(c['S'][s].copy())) for s in outside)      # bitwise untouched
    assert bool((r['big'][0::2] == GUARD).all()) and bool((r['big'][:, :, d:] == GUARD).all())           # and so is what lies between


@pytest.mark.parametrize('m,d,k,name', R.SHAPES, ids=[f'M{m}-d{d}-k{k}-{n}' for m, d, k, n in R.SHAPES])
def test_device_is_bitwise_the_host_twin(m, d, k, name):
    """Every kernel against its twin on the device's own inputs.  The perturbations alone are compared to a few ulp: they are
    logf / sincosf of the same Philox words in two libms, so the twin of prepare is then handed the device's draws."""
    slabs, lo, t = R.WINDOWS[2]
    c = R.case(m, d, k, name, slabs, lo, t, 1.05, 1.0)
    r = _device_analysis(c, name, lo, t, 1.0, 1.05, pad=0)
    Sh = np.array(c['S'])
    assert R.host_inflate(Sh, t, 1.05) == 0
    H = r['H'].cpu().numpy()
    own = R.host_weights(H, c['y'], 1.0, c['seed'], c['draw'])
    eps = r['eps'].cpu().numpy()
    assert np.abs(own['eps'] - eps).max() <= 4 * 2.0 ** -21
    w = R.host_weights(H, c['y'], 1.0, c['seed'], c['draw'], eps_in=eps)
    assert w['rcs'] == (0, 0, 0) and int(w['status'][0]) == 0 == int(r['status'])
    for nm in ('Y', 'D', 'part', 'W'):
        assert np.array_equal(r[nm].cpu().numpy().reshape(w[nm].shape), w[nm]), nm
    assert R.host_transform(Sh, lo, t, w['W']) == 0
    assert np.array_equal(r['S'][:slabs].cpu().numpy(), Sh)


def test_reproducible_and_independent_of_the_other_slabs():
    slabs, lo, t = R.WINDOWS[2]
    c = R.case(67, 512, 517, 'select', slabs, lo, t, 1.05, 1.0)
    first = _device_analysis(c, 'select', lo, t, 1.0, 1.05)
    again = _device_analysis(c, 'select', lo, t, 1.0, 1.05)
    shorter = _device_analysis(c, 'select', t - 1, t, 1.0, 1.05, extra=5)          # the last two slabs alone, in a longer tensor
    for nm in ('S', 'W', 'Y', 'D', 'part'):
        assert torch.equal(first[nm][:slabs] if nm == 'S' else first[nm], again[nm][:slabs] if nm == 'S' else again[nm]), nm
    assert torch.equal(first['W'], shorter['W']) and torch.equal(first['S'][t - 1:t + 1], shorter['S'][t - 1:t + 1])
    assert torch.equal(shorter['S'][:t - 1].cpu(), torch.from_numpy(c['S'][:t - 1].copy()))
    assert bool((shorter['S'][slabs:] == GUARD).all())


def test_an_infinite_observation_sets_the_status_and_leaves_the_window_untouched():
    c = R.case(15, 48, 5, 'select', 4, 1, 2, 1.0, 1.0)
    y = np.array(c['y'])
    y[2] = np.inf
    r = _device_analysis(c, 'select', 1, 2, 1.0, 1.0, y=y)
    assert int(r['status']) == 1 and not bool(r['W'].any())
    assert torch.equal(r['S'][:4].cpu(), torch.from_numpy(c['S'].copy()))


def _replay(record, out, y, A64, sigma, step, lag, inflation, seed, m):
    """Every analysis of a recorded enks_wide run against the float64 / float32 replays of its own recorded ensemble."""
    n = len(y)
    after = record['S'][1:] + [out]
    for i in range(n):
        t = (i + 1) * step
        lo = 0 if lag is None else max(0, t - lag * step)
        pre = record['S'][i].cpu().numpy()[:t + 1]
        k = y[i].numel()
        args = (pre, lo, t, A64, sigma, y[i].reshape(-1).cpu().numpy(), enks_ref.perturbations(m, k, seed, i), inflation)
        S64, S32 = R.analysis(*args, np.float64)[0], R.analysis(*args, np.float32)[0]
        got = after[i][:t + 1].double().cpu().numpy()
        err, tol = np.abs(got - S64).max(), bound(S32, S64)
        print(f'analysis {i}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (i, err, tol)
        assert np.array_equal(got[:lo], pre[:lo].astype(np.float64))                 # before the window: untouched


@pytest.mark.parametrize('m', [15, 64])
def test_enks_wide_beside_enks_fused_from_the_same_seed(m):
    """A shared case (d <= 64, k <= 64): one observation, so both routes analyse the same forecast with the same perturbations, and
    each is within its own bound of the same float64 reference."""
    from sda_amd import chains
    chain = chains.Lorenz96(n=8)
    obs = chains.AffineObservation(range(0, 8, 2), [0.0] * 4, [1.0] * 4)
    torch.manual_seed(3)
    step, sigma, inflation = 2, 0.5, 1.05
    x = chain.trajectory(chain.prior((m,), device='cuda'), 16, last=True)
    y = obs(chain.trajectory(x[:1], step)[-1, 0])[None] + sigma * torch.randn(1, 4, device='cuda')
    rf, rw = {}, {}
    fused = chains.enks_fused(chain, x, y, obs, sigma, step, inflation=inflation, seed=99, record=rf)
    wide = chains.enks_wide(chain, x, y, obs, sigma, step, inflation=inflation, seed=99, record=rw)
    assert wide.shape == fused.shape == (m, step + 1, 8) and rw['status'].tolist() == [0]
    y0, eps = y[0].cpu().numpy(), enks_ref.perturbations(m, 4, 99, 0)
    A = lambda v, dtype: enks_ref.obs_apply(v, obs.index, obs.shift, obs.scale, dtype)  # noqa: E731
    for nm, got, rec in (('fused', fused, rf), ('wide', wide, rw)):
        pre = rec['S'][0].cpu().numpy()                                            # the forecast the route analysed
        S64 = enks_ref.analysis(pre, 0, step, obs.index, obs.shift, obs.scale, sigma, y0, eps, inflation, np.float64)[0]
        if nm == 'fused':
            r32 = enks_ref.analysis(pre, 0, step, obs.index, obs.shift, obs.scale, sigma, y0, eps, inflation, np.float32)[0]
        else:
            r32 = R.analysis(pre, 0, step, A, sigma, y0, eps, inflation, np.float32)[0]
        err, tol = np.abs(got.permute(1, 0, 2).double().cpu().numpy() - S64).max(), bound(r32, S64)
        print(f'{nm}: err {err:.3e} bound {tol:.3e}')
        assert err <= tol, (nm, err, tol)
    assert (fused - wide).abs().max() < 1e-3                                       # and so of each other


@pytest.mark.parametrize('lag', [None, 1])
def test_enks_wide_on_the_kolmogorov_flow(lag):
    from sda_amd import chains, observe
    chain = chains.KolmogorovFlow(size=16, dt=0.2)
    m, n, step, sigma = 32, 3, 2, 0.1
    x = chain.prior((m,), device='cuda', seed=7)
    A = observe.Coarsen(2)
    truth = chain.trajectory(chain.prior((1,), device='cuda', seed=8), n * step)[step - 1::step, 0]
    torch.manual_seed(5)
    y = A(truth) + sigma * torch.randn(n, 2, 8, 8, device='cuda')
    record = {}
    out = chains.enks_wide(chain, x, y, A, sigma, step, lag=lag, seed=11, record=record)
    assert out.shape == (m, n * step + 1, 2, 16, 16) and bool(torch.isfinite(out).all())
    assert record['status'].tolist() == [0] * n and record['H'][0].shape == (m, 128) and record['W'][0].shape == (m, m)

    def A64(v, dtype):
        c = v.reshape(-1, 2, 8, 2, 8, 2)
        return ((c[:, :, :, 0, :, 0] + c[:, :, :, 0, :, 1] + c[:, :, :, 1, :, 0] + c[:, :, :, 1, :, 1]) * dtype(0.25)).reshape(-1, 128)
    _replay(record, out.transpose(0, 1).reshape(n * step + 1, m, -1), y, A64, sigma, step, lag, 1.0, 11, m)


def test_kolmogorov_enks_shape_and_time_convention():
    from sda_amd import chains, observe
    from sda_amd.experiments import kolmogorov
    chain = chains.KolmogorovFlow(size=16, dt=0.2)
    n, step, m = 2, 2, 8
    y = torch.zeros(n, 2, 8, 8, device='cuda')
    out = kolmogorov.enks(y, observe.Coarsen(2), 0.5, step, m, chain=chain, seed=3)
    assert out.shape == (m, (n - 1) * step + 1, 2, 16, 16) and bool(torch.isfinite(out).all())
    x = chain.prior((m,), device='cuda', seed=3)
    full = chains.enks_wide(chain, x, y, observe.Coarsen(2), 0.5, step, seed=3)
    assert torch.equal(out, full[:, step:])                               # the first returned state is the first observed one


def test_lorenz_enks_in_ensemble_space():
    from sda_amd import chains
    from sda_amd.experiments import lorenz
    torch.manual_seed(1)
    chain = chains.Lorenz96(40)
    A = lambda x: x[..., ::2]  # noqa: E731
    sigma, step, n_obs, m = 0.5, 2, 6, 128
    x = chain.trajectory(chain.prior((1,), device='cuda'), 64, last=True)
    truth = chain.trajectory(x, n_obs * step)[step - 1::step, 0]
    y = A(truth) + sigma * torch.randn(n_obs, 20, device='cuda')
    out = lorenz.enks(y, A, sigma, step, m, chain=chain, seed=5, space='ensemble')
    assert out.shape == (m, (n_obs - 1) * step + 1, 40) and bool(torch.isfinite(out).all())
    free = chain.trajectory(chain.trajectory(chain.prior((m,), device='cuda'), 64, last=True), n_obs * step).transpose(0, 1)[:, step - 1:]
    err_enks = (A(out[:, ::step]).mean(dim=0) - y).square().mean()
    err_free = (A(free[:, ::step]).mean(dim=0) - y).square().mean()
    print(f'mean-square misfit of the mean trajectory: enks {float(err_enks):.3f}, unconditioned forecast {float(err_free):.3f}')
    assert float(err_enks) < float(err_free)
    nonlinear = lorenz.enks(y.abs(), lambda x: x[..., ::2].abs(), sigma, step, m, chain=chain, seed=5, space='ensemble')
    assert nonlinear.shape == out.shape and bool(torch.isfinite(nonlinear).all())
