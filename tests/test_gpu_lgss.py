"""GPU: the linear-Gaussian state space (sda_amd/csrc/lgss.hip) -- the DampedSpring simulator, the exact posterior (filter, sampler,
evidence) and the exact score -- against the dense float64 reference of tests/lgss_ref.py, at the smallest shapes that reach each tail
(one lane, a partial wave, more than one workgroup; one tile of times, a partial tile, several tiles)."""
import functools

import numpy as np
import pytest
import torch

from sda_amd import chains, ops, parallel
from sda_amd.experiments import spring
from sda_amd.observe import Subsample
from sda_amd.score import VPSDE, DPSGaussianScore, GaussianScore
from tests import lgss_ref
from tests import lgss_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------- sda_lgss_advance
def test_advance_identity_returns_the_keyed_normals():
    model = ops.lgss_model(torch.zeros(8, 8), torch.zeros(8), torch.eye(8))
    x = torch.randn(130, 8, device=DEV)
    for d, mdl in ((8, model), (3, ops.lgss_model(torch.zeros(3, 3), torch.zeros(3), torch.eye(3)))):
        out = torch.empty(130, d, device=DEV)
        ops.lgss_advance(mdl, x[:, :d].contiguous(), out, 1, seed=77, row0=5, draw0=9)
        want = ops.randn_rows(torch.empty(130, d, device=DEV), 77, 5, draw=9)
        assert torch.equal(out, want)


@pytest.mark.parametrize('m', [1, 63, 65, 257])
@pytest.mark.parametrize('transitions', [1, 5])
def test_advance_spring_against_float64(m, transitions):
    """16 * 2^-24 (|b| + |A||x| + |Lq||z|) per transition (at most 8 + 8 rounded operations per row), carried through |A|."""
    chain = chains.DampedSpring()
    A, b, Q, _, _ = lgss_ref.spring()
    model = chain.model()
    Lq = np.array([[model.Lq[i][j] for j in range(4)] for i in range(4)], np.float64)
    wide = torch.randn(m, 6, device=DEV)
    x = wide[:, 1:5]                                                 # a non-contiguous view: row stride 6
    seed, draw0 = 31, 4
    every = torch.empty(transitions, m, 4, device=DEV)
    ops.lgss_advance(model, x, every, transitions, every=True, out_st=m * 4, seed=seed, draw0=draw0)
    last = torch.empty(m, 4, device=DEV)
    ops.lgss_advance(model, x, last, transitions, seed=seed, draw0=draw0)
    assert torch.equal(last, every[-1])
    ref, bound = x.double().cpu().numpy(), np.zeros((m, 4))
    for t in range(transitions):
        z = ops.randn_rows(torch.empty(m, 4, device=DEV), seed, 0, draw=draw0 + t).double().cpu().numpy()
        bound = bound @ np.abs(A).T + 16 * 2.0 ** -24 * (np.abs(b) + np.abs(ref) @ np.abs(A).T + np.abs(z) @ np.abs(Lq).T)
        ref = ref @ A.T + b + z @ Lq.T
        err = np.abs(every[t].double().cpu().numpy() - ref)
        assert (err <= bound).all(), (t, (err / bound).max())


def test_chain_seed_reproduces_and_draws_advance():
    chain = chains.DampedSpring()
    x = chain.prior((65,), device=DEV)
    a = chain.trajectory(x, 3, seed=5)
    assert a.shape == (3, 65, 4) and chain._draw == 3
    chain2 = chains.DampedSpring()
    assert torch.equal(chain2.trajectory(x, 3, seed=5), a)
    assert torch.equal(chains.DampedSpring().trajectory(x, 3, last=True, seed=5), a[-1])
    # two successive calls of ONE chain do not reuse noise: the second transition from the same state and seed differs from the first
    chain3 = chains.DampedSpring()
    first, second = chain3.transition(x, seed=5), chain3.transition(x, seed=5)
    assert not torch.equal(first, second) and torch.equal(first, a[0])
    assert chain3.transition(x.reshape(5, 13, 4), seed=5).shape == (5, 13, 4)


# ---------------------------------------------------------------- sda_lgss_filter
def _case(d):
    return {1: U.random_case(1, 1, 11), 4: U.spring_case(k=1, sigma=0.05, step=1), 8: U.random_case(8, 3, 7)}[d]


@pytest.mark.parametrize('d', [1, 4, 8])
@pytest.mark.parametrize('N,step', [(1, 1), (2, 3), (9, 8)])
@pytest.mark.parametrize('B', [1, 3])
def test_filter_against_dense_conditioning(d, N, step, B):
    case = _case(d)
    A, b, Q, m0, P0, H, c, sigma = case
    k, T = len(c), (N - 1) * step
    y = U.observations(case, step, N, B, seed=N + B)
    m64 = U.model64(case)
    table = ops.lgss_tables(m64, step, N, device=DEV)
    mean, logz = ops.lgss_filter(m64, table, _t(y).to(DEV), step)
    assert mean.shape == (B, T + 1, d) and mean.dtype == torch.float64
    for s in range(B):
        _, _, mf, _ = lgss_ref.tables_posterior(table.cpu().numpy(), d, k, T, step, A, b, H, c, m0, y[s].astype(np.float64))
        want_logz = U.dense_posterior(case, step, y[s])[2]
        # the filtered mean at the LAST index is the posterior mean there: dense conditioning checks it independently of the tables
        post = U.dense_posterior(case, step, y[s])[0].reshape(T + 1, d)
        got = mean[s].cpu().numpy()
        assert np.abs(got - mf).max() <= 1e-9 * np.abs(mf).max()
        assert np.abs(got[T] - post[T]).max() <= 1e-9 * np.abs(post).max()
        assert abs(float(logz[s]) - want_logz) <= 1e-9 * max(abs(want_logz), 1.0)


# ---------------------------------------------------------------- sda_lgss_sample
@pytest.mark.parametrize('T', [0, 3, 64])
@pytest.mark.parametrize('B', [1, 3])
def test_sampler_against_the_float64_recursions(T, B):
    """Every sample = the float64 evaluation of the two recursions on the same normals, to 2^-22 max|x|; and sample (b, r) does not
    depend on M or B."""
    step = {0: 1, 3: 3, 64: 8}[T]
    N = T // step + 1
    case = U.spring_case(k=1, sigma=0.05, step=step)
    A, b = case[0], case[1]
    y = U.observations(case, step, N, B, seed=T)
    m64 = U.model64(case)
    table = ops.lgss_tables(m64, step, N, device=DEV)
    mean, _ = ops.lgss_filter(m64, table, _t(y).to(DEV), step)
    seed, draw0 = 1234, 2
    outs = {}
    for M in (1, 63, 65, 257):
        out = ops.lgss_sample(m64, table, mean, M, seed, draw0=draw0)
        assert out.shape == (B, M, T + 1, 4)
        z = lambda i: ops.randn_rows(torch.empty(B * M, 4, device=DEV), seed, 0, draw=draw0 + i).double().cpu().numpy()
        want = U.sample_ref(table.cpu().numpy(), 4, 1, T, A, b, mean.cpu().numpy(), M, z)
        assert np.abs(out.double().cpu().numpy() - want).max() <= 2.0 ** -22 * np.abs(want).max()
        outs[M] = out
    # row b * M + r: sequence 0 of the M = 257 launch shares rows 0 .. 62 with the M = 63 one, and a B = 1 launch with the B = 3 one
    assert torch.equal(outs[257][0, :63], outs[63][0]) and torch.equal(outs[65][0, :1], outs[1][0])
    if B == 3:
        one = ops.lgss_sample(m64, table, mean[:1].contiguous(), 65, seed, draw0=draw0)
        assert torch.equal(one[0], outs[65][0])


def test_posterior_in_law():
    """M = 4096 exact samples of the `lo` configuration (N = 9, step = 8, k = 1, sigma = 0.05): every component of the empirical mean
    within 5 standard errors of the exact mean, every empirical variance within 5 sqrt(2 / M) relative of the exact one.  Deterministic
    at a fixed seed; the dense reference's own numpy draws at this width pass the same two checks with margin."""
    M = 4096
    case = U.spring_case(k=1, sigma=0.05, step=8)
    y = _t(U.observations(case, 8, 9, 1, seed=2)[0])
    A_obs = lambda x: x[..., :1]
    x = spring.posterior(y, A_obs, 0.05, 8, M, seed=20240)
    assert x.shape == (M, 65, 4) and x.dtype == torch.float32 and x.is_cuda
    mean, cov, cross = spring.posterior_moments(y, A_obs, 0.05, 8)
    dense_mean, dense_cov, dense_logz = U.dense_posterior(case, 8, y.numpy())
    assert np.abs(mean.numpy().reshape(-1) - dense_mean).max() <= 1e-9 * np.abs(dense_mean).max()
    var = torch.diagonal(cov, dim1=1, dim2=2)
    assert np.abs(var.numpy().reshape(-1) - np.diag(dense_cov)).max() <= 1e-9 * np.abs(dense_cov).max()
    assert np.abs(cross[5].numpy() - dense_cov[20:24, 24:28]).max() <= 1e-9 * np.abs(dense_cov).max()
    xs = x.double().cpu()
    emp_mean, emp_var = xs.mean(0), xs.var(0, unbiased=True)
    zscore = ((emp_mean - mean) / (var / M).sqrt()).abs().max()
    vdev = (emp_var / var - 1).abs().max()
    print(f'posterior in law: max |z| of the mean {float(zscore):.3f} (bound 5), max relative variance error {float(vdev):.4f} '
          f'(bound {5 * (2 / M) ** 0.5:.4f})')
    assert zscore <= 5 and vdev <= 5 * (2 / M) ** 0.5
    logz = spring.log_evidence(y, A_obs, 0.05, 8)
    assert abs(float(logz) - dense_logz) <= 1e-9 * abs(dense_logz)
    batched = spring.posterior(torch.stack((y, y)), A_obs, 0.05, 8, 3, seed=1)
    assert batched.shape == (2, 3, 65, 4)
    with pytest.raises(Exception):
        spring.posterior(y, lambda x: x[..., :1] ** 2, 0.05, 8, 3)


# ---------------------------------------------------------------- ExactScore
@functools.lru_cache(maxsize=None)
def _dense_prior(length):
    A, b, Q, m0, P0 = U.spring_case(step=1)[:5]
    return lgss_ref.precision(A, Q, P0, length - 1), lgss_ref.joint(A, b, Q, m0, P0, length - 1)[0]


@pytest.mark.parametrize('length', [1, 2, 9, 65])
@pytest.mark.parametrize('batch', [1, 65, 300])
def test_exact_score_against_the_dense_solve(length, batch):
    score = spring.ExactScore(spring.make_chain(), length)
    Lam, m = _dense_prior(length)
    torch.manual_seed(length * 1000 + batch)
    x = torch.randn(batch, length, 4).to(DEV)
    g = torch.randn(batch, length, 4).to(DEV)
    outs = []
    for t in (1.0, 0.5, 0.0):
        tt = torch.tensor(t, device=DEV)
        mu, sigma = (float(v) for v in score._schedule(tt).cpu())
        xg = x.clone().requires_grad_(True)
        eps = score(xg, tt)
        want = lgss_ref.eps_dense(x.double().cpu().numpy().reshape(batch, -1), mu, sigma, Lam, m)
        assert np.abs(eps.detach().double().cpu().numpy().reshape(batch, -1) - want).max() <= 2.0 ** -22 * np.abs(want).max()
        # the Jacobian is symmetric: the gradient of (eps * g).sum() is the module applied to g around a zero mean
        grad, = torch.autograd.grad((eps * g).sum(), xg)
        want_g = lgss_ref.eps_dense(g.double().cpu().numpy().reshape(batch, -1), mu, sigma, Lam, 0 * m)
        assert np.abs(grad.double().cpu().numpy().reshape(batch, -1) - want_g).max() <= 2.0 ** -22 * np.abs(want_g).max()
        outs.append(eps.detach())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])      # (each call used its own factor)
    assert torch.equal(score(x, torch.tensor(1.0, device=DEV)), outs[0])


# ---------------------------------------------------------------- guided sampler on an analytic score
@pytest.mark.parametrize('kind', ['gaussian', 'dps'])
def test_guided_sampler_on_the_analytic_score(kind):
    """The guided predictor-corrector loop with the analytic score against a float64 replay on the same noise table.  Bound (the
    project's standing rule): at most 4 times the error a float32 torch-CPU replay of the same loop makes against the float64 one."""
    L, n, steps = 65, 4, 8
    case = U.spring_case(k=1, sigma=0.05, step=8)
    A, b, Q, m0, P0 = case[:5]
    y = _t(U.observations(case, 8, 9, 1, seed=4)[0])                  # (9, 1)
    gen = torch.Generator().manual_seed(99)
    x0 = torch.randn(n, L, 4, generator=gen)
    noise = torch.randn(steps, n, L, 4, generator=gen)
    sel = (slice(None, None, 8), slice(0, 1))
    obs = Subsample(sel)

    def make():
        inner = VPSDE(spring.ExactScore(spring.make_chain(), L, step=8), shape=())
        if kind == 'gaussian':
            guide = GaussianScore(y, obs, std=0.05, sde=inner, gamma=3e-2)
        else:
            guide = DPSGaussianScore(y, obs, sde=inner, zeta=1.0)
        sde = VPSDE(guide, shape=(L, 4)).to(DEV)
        sde.initial_noise = x0
        sde.noise_source = parallel.TableNoise(noise.to(DEV), 1)
        return sde

    def run(capture):
        sampler = make().sampler((n,), steps=steps, corrections=1, tau=0.25)
        if capture:
            sampler.capture()
        for _ in range(steps):
            sampler.step()
        return sampler.result()

    got = run(False)
    Lam, m = lgss_ref.precision(A, Q, P0, L - 1), lgss_ref.joint(A, b, Q, m0, P0, L - 1)[0]
    kw = dict(dps_zeta=1.0) if kind == 'dps' else {}
    ref64 = lgss_ref.pc_replay(x0, steps, 1, 0.25, noise, lgss_ref.guided_score(Lam, m, y, 0.05, 3e-2, sel, torch.float64, **kw), torch.float64)
    ref32 = lgss_ref.pc_replay(x0, steps, 1, 0.25, noise, lgss_ref.guided_score(Lam, m, y, 0.05, 3e-2, sel, torch.float32, **kw), torch.float32)
    err = float((got.double().cpu() - ref64).abs().max())
    yard = float((ref32.double() - ref64).abs().max())
    print(f'guided sampler ({kind}): device vs float64 replay {err:.3e}, float32 torch-CPU replay vs float64 {yard:.3e}, '
          f'max |x| {float(ref64.abs().max()):.3f}')
    assert err <= 4 * yard
    assert torch.equal(run(True), got)                               # the captured step replays the uncaptured one bitwise
