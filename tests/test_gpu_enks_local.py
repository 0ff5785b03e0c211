"""GPU: the domain-localised smoother kernels (csrc/enks_local.hip) against the float64 numpy replay (tests/enks_local_ref.py) under
the project's bound rule, bitwise against their host twins, their locality, reproducibility and slab independence, the reduction to
``enks_wide``'s analysis, ``chains.enks_local`` on the Kolmogorov flow with every analysis replayed, and the experiment entries."""
import numpy as np
import pytest
import torch

from tests import enks_ref
from tests import enks_local_ref as R
from tests import enks_wide_ref as RW
from tests.chain_util import bound

pytestmark = pytest.mark.gpu

GUARD = 12345.0


def _device_analysis(c, A, plan, lo, t, sigma, inflation, *, extra=0, pad=3, y=None):
    """The ops on a time-strided, member-padded view of a larger tensor: dict(S, big, H, Y, D, eps, W, status)."""
    from sda_amd import ops
    S0 = c['S']
    slabs, m, d = S0.shape
    big = torch.full((2 * (slabs + extra) + 1, m, d + pad), GUARD, device='cuda')
    S = big[1::2, :, :d]
    S[:slabs] = torch.from_numpy(S0.copy()).cuda()
    ops.enkw_inflate(S, t, inflation)
    k = c['y'].shape[0]
    H = A(S[t].contiguous()).reshape(m, k).contiguous()
    yd = torch.from_numpy(np.array(c['y'] if y is None else y)).cuda()
    Y, D, eps = ops.enkw_prepare(H, yd, sigma, seed=c['seed'], draw=c['draw'])
    W, status = ops.enkl_weights(plan, Y, D, sigma)
    ops.enkl_transform(plan, S, lo, t, W)
    return dict(S=S, big=big, H=H, Y=Y, D=D, eps=eps, W=W, status=status)


def _case(m, event, block, name, radius, slabs, lo, t, inflation, sigma):
    from sda_amd import ops
    c = R.case(m, event, block, name, radius, slabs, lo, t, inflation, sigma)
    plan = ops.enkl_plan(event, c['pos'], radius, block)
    assert np.array_equal(plan.offsets.cpu().numpy(), c['P']['offsets'])
    return c, plan, R.device_operator(name, event)[1]


@pytest.mark.parametrize('m,event,block,name,radius,window,inflation,sigma', R.CASES, ids=R.IDS)
def test_ops_match_the_float64_replay(m, event, block, name, radius, window, inflation, sigma):
    slabs, lo, t = window
    c, plan, A = _case(m, event, block, name, radius, slabs, lo, t, inflation, sigma)
    r = _device_analysis(c, A, plan, lo, t, sigma, inflation)
    assert not bool(r['status'].any())
    (S64, H64, W64), (S32, H32, W32) = c['ref64'], c['ref32']
    S = r['S'][:slabs]
    for nm, got, r32, r64 in (('W', R.acting(r['W'].cpu().numpy(), sigma), R.acting(W32, sigma), R.acting(W64, sigma)),
                              ('S', S[lo:t + 1].double().cpu().numpy(), S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got - r64).max(), bound(r32, r64)
        print(f'{nm}: err {err:.3e} bound {tol:.3e} ratio {err / tol:.3f}')
        assert err <= tol, (nm, err, tol)
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(torch.equal(S[s].cpu(), torch.from_numpy(c['S'][s].copy())) for s in outside)      # bitwise untouched
    assert bool((r['big'][0::2] == GUARD).all()) and bool((r['big'][:, :, int(np.prod(event)):] == GUARD).all())


@pytest.mark.parametrize('m,event,block,name,radius,sigmas', R.SHAPES, ids=R.SHAPE_IDS)
def test_device_is_bitwise_the_host_twin(m, event, block, name, radius, sigmas):
    """The pack, the per-block solve and the update against their twins on the device's own Y, D."""
    slabs, lo, t = R.WINDOWS[2]
    c, plan, A = _case(m, event, block, name, radius, slabs, lo, t, 1.05, 1.0)
    r = _device_analysis(c, A, plan, lo, t, 1.0, 1.05, pad=0)
    w = R.host_weights(c['P'], None, None, 1.0, 0, 0, Y=r['Y'].cpu().numpy(), D=r['D'].cpu().numpy())
    assert w['rcs'] == (0, 0) and not w['status'].any() and not bool(r['status'].any())
    assert np.array_equal(r['W'].cpu().numpy(), w['W'])
    Sh = np.array(c['S'])
    assert RW.host_inflate(Sh, t, 1.05) == 0 and R.host_transform(c['P'], Sh, lo, t, w['W']) == 0
    assert np.array_equal(r['S'][:slabs].cpu().numpy(), Sh)


REDUCTIONS = [(15, 48, 5, 'select', (1, 1, 48)), (17, 200, 300, 'select', (1, 1, 200)), (128, 512, 64, 'vortcoarse', (2, 16, 16))]


@pytest.mark.parametrize('m,d,k,name,event', REDUCTIONS, ids=[f'M{r[0]}-d{r[1]}-k{r[2]}' for r in REDUCTIONS])
def test_one_block_with_an_infinite_radius_is_within_the_bound_of_the_global_reference(m, d, k, name, event):
    from sda_amd import ops
    slabs, lo, t = R.WINDOWS[2]
    c = RW.case(m, d, k, name, slabs, lo, t, 1.05, 1.0)
    plan = ops.enkl_plan(event, np.zeros((k, 2)), float('inf'), event[1:])
    assert plan.nblk == 1
    r = _device_analysis(c, RW.device_operator(name, d, k), plan, lo, t, 1.0, 1.05)
    S64, S32 = c['ref64'][0], c['ref32'][0]
    err, tol = np.abs(r['S'][lo:t + 1].double().cpu().numpy() - S64[lo:t + 1]).max(), bound(S32[lo:t + 1], S64[lo:t + 1])
    print(f'S: err {err:.3e} bound {tol:.3e}')
    assert int(r['status']) == 0 and err <= tol


def test_an_empty_list_leaves_its_block_untouched():
    m, event, block, name, radius, _ = R.SHAPES[0]
    c, plan, A = _case(m, event, block, name, radius, 4, 1, 2, 1.0, 1.0)
    r = _device_analysis(c, A, plan, 1, 2, 1.0, 1.0)
    P = c['P']
    S, W = r['S'][:4].cpu().numpy(), r['W'].cpu().numpy()
    for b in range(P['nblk']):
        empty = P['offsets'][b] == P['offsets'][b + 1]
        assert np.array_equal(S[:, :, P['comps'][b]], c['S'][:, :, P['comps'][b]]) == empty and bool(W[b].any()) != empty
    assert not bool(r['status'].any())


@pytest.mark.parametrize('shape', [R.SHAPES[1], R.SHAPES[6]], ids=[R.SHAPE_IDS[1], R.SHAPE_IDS[6]])
def test_an_observation_reaches_only_the_blocks_that_list_it(shape):
    m, event, block, name, radius, _ = shape
    slabs, lo, t = R.WINDOWS[1]
    c, plan, A = _case(m, event, block, name, radius, slabs, lo, t, 1.0, 1.0)
    P = c['P']
    i0 = int(P['idx'][len(P['idx']) // 2])
    listing = R.blocks_listing(P, i0)
    assert 0 < len(listing) < P['nblk']
    base = _device_analysis(c, A, plan, lo, t, 1.0, 1.0)
    S0, W0 = base['S'][:slabs].cpu().numpy(), base['W'].cpu().numpy()
    for value in (float(c['y'][i0]) + 1.0, np.inf):
        y = np.array(c['y'])
        y[i0] = value
        r = _device_analysis(c, A, plan, lo, t, 1.0, 1.0, y=y)
        S, W = r['S'][:slabs].cpu().numpy(), r['W'].cpu().numpy()
        assert r['status'].tolist() == [int(not np.isfinite(value) and b in listing) for b in range(P['nblk'])]
        for b in range(P['nblk']):
            comp = P['comps'][b]
            if b not in listing:
                assert np.array_equal(W[b], W0[b]) and np.array_equal(S[:, :, comp], S0[:, :, comp])
            elif np.isfinite(value):
                assert not np.array_equal(W[b], W0[b]) and not np.array_equal(S[:, :, comp], S0[:, :, comp])
            else:
                assert not W[b].any() and np.array_equal(S[:, :, comp], c['S'][:, :, comp])


def test_reproducible_and_independent_of_the_other_slabs():
    m, event, block, name, radius, _ = R.SHAPES[8]
    slabs, lo, t = R.WINDOWS[2]
    c, plan, A = _case(m, event, block, name, radius, slabs, lo, t, 1.05, 1.0)
    first = _device_analysis(c, A, plan, lo, t, 1.0, 1.05)
    again = _device_analysis(c, A, plan, lo, t, 1.0, 1.05)
    shorter = _device_analysis(c, A, plan, t - 1, t, 1.0, 1.05, extra=5)           # the last two slabs alone, in a longer tensor
    assert torch.equal(first['S'][:slabs], again['S'][:slabs]) and torch.equal(first['W'], again['W'])
    assert torch.equal(first['W'], shorter['W']) and torch.equal(first['S'][t - 1:t + 1], shorter['S'][t - 1:t + 1])
    assert torch.equal(shorter['S'][:t - 1].cpu(), torch.from_numpy(c['S'][:t - 1].copy()))
    assert bool((shorter['S'][slabs:] == GUARD).all())


def _replay(record, out, y, A64, pos, radius, block, sigma, step, lag, inflation, seed, m):
    """Every analysis of a recorded enks_local run against the float64 / float32 replays of its own recorded ensemble."""
    n = len(y)
    after = record['S'][1:] + [out]
    plan = record['plan']
    P = R.plan(plan.event, pos, radius, block)
    for i in range(n):
        t = (i + 1) * step
        lo = 0 if lag is None else max(0, t - lag * step)
        pre = record['S'][i].cpu().numpy()[:t + 1]
        k = y[i].numel()
        args = (pre, lo, t, A64, sigma, y[i].reshape(-1).cpu().numpy(), enks_ref.perturbations(m, k, seed, i), inflation, P)
        (S64, _, W64), (S32, _, W32) = R.analysis(*args, np.float64), R.analysis(*args, np.float32)
        got = after[i][:t + 1].double().cpu().numpy()
        for nm, g, r32, r64 in (('S', got, S32, S64), ('W', record['W'][i].double().cpu().numpy(), W32, W64)):
            err, tol = np.abs(g - r64).max(), bound(r32, r64)
            print(f'analysis {i} {nm}: err {err:.3e} bound {tol:.3e}')
            assert err <= tol, (i, nm, err, tol)
        assert np.array_equal(got[:lo], pre[:lo].astype(np.float64))                 # before the window: untouched


@pytest.mark.parametrize('lag', [None, 1])
def test_enks_local_on_the_kolmogorov_flow(lag):
    from sda_amd import chains, observe
    chain = chains.KolmogorovFlow(size=16, dt=0.2)
    m, n, step, sigma, radius, block = 32, 3, 2, 0.1, 4.0, (4, 4)
    x = chain.prior((m,), device='cuda', seed=7)
    A = observe.Coarsen(2)
    truth = chain.trajectory(chain.prior((1,), device='cuda', seed=8), n * step)[step - 1::step, 0]
    torch.manual_seed(5)
    y = A(truth) + sigma * torch.randn(n, 2, 8, 8, device='cuda')
    record = {}
    pos = observe.positions(A, (2, 16, 16))
    out = chains.enks_local(chain, x, y, A, sigma, step, positions=pos, radius=radius, block=block, lag=lag, seed=11, record=record)
    assert out.shape == (m, n * step + 1, 2, 16, 16) and bool(torch.isfinite(out).all())
    assert tuple(record['status'].shape) == (n, 16) and not bool(record['status'].any())
    assert record['H'][0].shape == (m, 128) and record['W'][0].shape == (16, m, m)
    _replay(record, out.transpose(0, 1).reshape(n * step + 1, m, -1), y, R.operator('coarsen', (2, 16, 16)), pos, radius, block, sigma,
            step, lag, 1.0, 11, m)


def test_kolmogorov_enks_with_and_without_a_radius():
    from sda_amd import chains, observe
    from sda_amd.experiments import kolmogorov
    chain = chains.KolmogorovFlow(size=16, dt=0.2)
    n, step, m = 2, 2, 8
    y = torch.zeros(n, 2, 8, 8, device='cuda')
    x = chain.prior((m,), device='cuda', seed=3)
    present = chains.enks_wide(chain, x, y, observe.Coarsen(2), 0.5, step, seed=3)[:, step:]
    assert torch.equal(kolmogorov.enks(y, observe.Coarsen(2), 0.5, step, m, chain=chain, seed=3, radius=None), present)
    out = kolmogorov.enks(y, observe.Coarsen(2), 0.5, step, m, chain=chain, seed=3, radius=4.0)
    assert out.shape == (m, (n - 1) * step + 1, 2, 16, 16) and bool(torch.isfinite(out).all())
    full = chains.enks_local(chain, x, y, observe.Coarsen(2), 0.5, step, positions=observe.positions(observe.Coarsen(2), (2, 16, 16)),
                             radius=4.0, block=(4, 4), seed=3)
    assert torch.equal(out, full[:, step:]) and not torch.equal(out, present)


L96_STEP, L96_RADIUS = 2, 2.0


def test_localisation_tracks_lorenz96_where_the_global_analysis_diverges():
    """Lorenz96(40) (F = 16, dt = 0.01), every other component observed, sigma = 0.5, 16 members, blocks of 4, inflation 1.05, lag 0,
    40 observations of which the last 30 are scored, 4 seeds pooled: the RMS error of the localised run's ensemble mean is below
    sigma and below half the global run's.

    step = 2 and radius = 2 come from the float64 numpy replay on this chain's transitions (profiles/enks_local_parity.txt): there
    every one of 4 seeds ends at 0.28 .. 0.38 localised against 5.5 .. 10.5 global.  At radius 4 (and 3) one seed of the four
    diverged in the replay (4.3; the other three 0.26 .. 0.31), which is marginal, so the radius was lowered and the conditions
    were kept."""
    from sda_amd import chains
    from sda_amd.experiments import lorenz
    chain = chains.Lorenz96(40)
    A = lambda x: x[..., ::2]  # noqa: E731
    sigma, n_obs, m, step = 0.5, 40, 16, L96_STEP
    sq = {'local': [], 'global': []}
    for seed in range(4):
        torch.manual_seed(100 + seed)
        x = chain.trajectory(chain.prior((1,), device='cuda'), 64, last=True)
        truth = chain.trajectory(x, n_obs * step)[step - 1::step, 0]
        y = A(truth) + sigma * torch.randn(n_obs, 20, device='cuda')
        for name, radius in (('local', L96_RADIUS), ('global', None)):
            torch.manual_seed(200 + seed)
            out = lorenz.enks(y, A, sigma, step, m, chain=chain, seed=seed, space='ensemble', radius=radius, block=4, inflation=1.05, lag=0)
            assert out.shape == (m, (n_obs - 1) * step + 1, 40)
            err = (out[:, ::step].mean(dim=0) - truth)[-30:].square().mean()
            sq[name].append(float(err))
            print(f'seed {seed} {name}: RMS {float(err) ** 0.5:.3f}')
    rms = {k: float(np.sqrt(np.mean(v))) for k, v in sq.items()}
    print(f'pooled RMS: localised {rms["local"]:.3f}, global {rms["global"]:.3f}, sigma {sigma}')
    assert rms['local'] < sigma and rms['local'] < 0.5 * rms['global']
