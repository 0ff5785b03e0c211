"""GPU: the Markov-chain and particle-filter kernels (sda_amd/csrc/chain.hip) and the Python layer on top of them
(sda_amd.chains, sda_amd.experiments.lorenz) against the reference's own outputs (tests/golden/chains.npz) and the numpy
restatement tests/chain_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains, ops
from sda_amd.experiments import lorenz
from tests import chain_ref
from tests import chain_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567890abcdef


@pytest.fixture(scope='module')
def dev():
    _lib.load()
    return torch.device('cuda:0')


def _tile(a, m, axis):
    """The fixture's 7 states repeated to m along `axis`."""
    idx = np.arange(m) % a.shape[axis]
    return np.take(a, idx, axis=axis)


@pytest.mark.parametrize('key', list(U.CHAINS))
def test_transitions_and_trajectories(dev, key):
    """Every chain of the fixture at m = 1, 7, 65, 1000 (partial waves, partial Lorenz-96 sub-groups; n = 5 and n = 40 are
    non-power-of-two sub-groups) against the reference run in float64, bound = max(1e-6 max|x|, 3 x the reference's own fp32
    error).  last=True is the last row of last=False and a strided output equals the contiguous one, bit for bit."""
    g = U.golden()
    chain = U.make(key)
    b1 = U.bound(g[f'{key}/trans32'], g[f'{key}/trans64'])
    bn = U.bound(g[f'{key}/traj32'], g[f'{key}/traj64'])
    for m in (1, 7, 65, 1000):
        x = torch.from_numpy(_tile(g[f'{key}/x0'], m, 0)).to(dev)
        one = chain.transition(x)
        traj = chain.trajectory(x, 16)
        last = chain.trajectory(x, 16, last=True)
        assert one.shape == x.shape and traj.shape == (16, *x.shape) and last.shape == x.shape
        assert np.abs(one.cpu().numpy() - _tile(g[f'{key}/trans64'], m, 0)).max() <= b1, (key, m)
        assert np.abs(traj.cpu().numpy() - _tile(g[f'{key}/traj64'], m, 1)).max() <= bn, (key, m)
        assert torch.equal(last, traj[-1]) and torch.equal(one, traj[0])
        d = x.shape[1]
        buf = torch.full((m, 18, d + 3), 7.0, device=dev)           # (m, time, padded d): the transposed, padded layout
        ops.chain_advance(chain.model(), x, buf.reshape(-1)[d + 3:], 16, every=True,
                          out_st=d + 3, out_sp=18 * (d + 3))
        assert torch.equal(buf[:, 1:17, :d], traj.transpose(0, 1))
        assert (buf[:, 0] == 7).all() and (buf[:, 17] == 7).all() and (buf[:, :, d:] == 7).all()
    xb = torch.from_numpy(g[f'{key}/x0']).to(dev).reshape(7, 1, -1).expand(7, 2, -1)      # batch shape (7, 2), non-contiguous
    assert torch.equal(chain.trajectory(xb, 3)[:, :, 1], chain.trajectory(xb[:, 0].contiguous(), 3))


def test_noise(dev):
    g = U.golden()
    chain = chains.NoisyLorenz63(dt=0.025)
    x0 = g['l63/x0']
    x = torch.from_numpy(x0).to(dev)
    got = chain.trajectory(x, 5, seed=SEED)                          # draws 0 .. 4 of a fresh chain
    ref = chain_ref.trajectory(*U.ref_args(chain), x0.astype(np.float64), 5, 0.025 ** 0.5, SEED, 0, 0)
    assert np.abs(got.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
    # geometry independence: 1000 particles in one launch = two launches of 500 with row0 0 and 500, bit for bit
    xs = chain.prior((1000,), device=dev)
    model = chain.model()
    whole = ops.chain_advance(model, xs, torch.empty(3, 1000, 3, device=dev), 3, every=True, out_st=3000, seed=SEED, draw0=9)
    lo = ops.chain_advance(model, xs[:500], torch.empty(3, 500, 3, device=dev), 3, every=True, out_st=1500, seed=SEED, draw0=9)
    hi = ops.chain_advance(model, xs[500:], torch.empty(3, 500, 3, device=dev), 3, every=True, out_st=1500, seed=SEED, row0=500, draw0=9)
    assert torch.equal(whole, torch.cat((lo, hi), dim=1))
    # successive calls never reuse noise: same seed, the draw counter moved on; and without a seed torch's generator decides
    a, b = chain.transition(x, seed=SEED), chain.transition(x, seed=SEED)
    assert not torch.equal(a, b)
    torch.manual_seed(3)
    c = chains.NoisyLorenz63(dt=0.025).transition(x)
    torch.manual_seed(3)
    d = chains.NoisyLorenz63(dt=0.025).transition(x)
    assert torch.equal(c, d) and not torch.equal(c, chains.NoisyLorenz63(dt=0.025).transition(x))
    mean, std = chain.moments(x)
    assert torch.equal(mean, chains.Lorenz63(dt=0.025).transition(x)) and std == 0.025 ** 0.5


def test_log_prob_log_prior_log_likelihood(dev):
    """Against the float64 fixture to 1e-5 of the array's largest magnitude (see tests/test_chains_host.py for why per array)."""
    g = U.golden()
    chain = lorenz.make_chain()
    x, y = torch.from_numpy(g['lp/x']).to(dev), torch.from_numpy(g['lp/y']).to(dev)
    A = lambda v: chain.preprocess(v)[..., :1]      # noqa: E731
    for got, key in ((chain.log_prob(x[:, :-1], x[:, 1:]), 'log_prob64'), (lorenz.log_prior(x), 'log_prior64'),
                     (lorenz.log_likelihood(y, x, A=A, sigma=0.25, step=2), 'log_lik64')):
        ref = g[f'lp/{key}']
        assert got.shape == ref.shape
        assert np.abs(got.double().cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max(), key
    # the differentiable route (weak_4d_var) agrees with the kernel and has a gradient
    xg = x.clone().requires_grad_()
    lp = lorenz.log_prior(xg)
    lp.sum().backward()
    assert torch.allclose(lp.detach(), lorenz.log_prior(x), rtol=1e-4) and torch.isfinite(xg.grad).all()
    out = lorenz.weak_4d_var(x[0], y[0], A=A, sigma=0.25, step=2, iterations=2)
    assert out.shape == x[0].shape and torch.isfinite(out).all()


def _weights_case(dev, m, index, shift, scale, sigma, x=None, y=None):
    chain = lorenz.make_chain()
    torch.manual_seed(m)
    x = chain.prior((m,), device=dev) if x is None else x.to(dev)
    obs_fn = chains.AffineObservation(index, shift, scale)
    y = (obs_fn(x[0]) + 0.1).float() if y is None else y.to(dev)
    o = ops.chain_obs(index, shift, scale, sigma, y.contiguous())
    logw, pmax = ops.bpf_logweights(x, o)
    ref = torch.softmax(torch.distributions.Normal(y.double(), sigma).log_prob(obs_fn(x.double())).sum(-1), 0)
    return x, logw, pmax, ref


@pytest.mark.parametrize('m,index,shift,scale', [(1, [0], [0.0], [8.0]), (65, [0, 2], [0.0, 25.0], [8.0, 8.6]), (5000, [0], [0.0], [8.0])])
def test_weights_and_resampling(dev, m, index, shift, scale):
    """w / sum w against torch.softmax of the float64 log-likelihood to 1e-5 of the largest weight; the float64 prefix sums; the
    ancestors against chain_ref's searchsorted replay of the device's OWN fp32 w.  5000 particles are five chunks of the cdf
    kernel's 1024-thread workgroup."""
    x, logw, pmax, ref = _weights_case(dev, m, index, shift, scale, 0.25)
    for pm in (pmax, None):
        w, cdf, status = ops.bpf_cdf(logw, pm)
        assert int(status) == 0
        wn = w.double() / w.double().sum()
        assert (wn - ref).abs().max() <= 1e-5 * ref.max()
        assert float(w.max()) == 1.0
    wh = w.cpu().numpy()
    assert np.abs(cdf.cpu().numpy() - np.cumsum(wh.astype(np.float64))).max() <= 1e-13 * wh.astype(np.float64).sum()
    for obs_index in (0, 3):
        anc = ops.bpf_resample(cdf, SEED, obs_index).cpu().numpy()
        want, _, _, margin = chain_ref.ancestors(wh, SEED, obs_index, return_margin=True)
        assert (margin <= 1e-12).sum() == 0                          # the replay alone has no draw on a boundary
        diff = np.nonzero(anc != want)[0]
        assert len(diff) <= 1 and (margin[diff] <= 1e-12).all(), (diff, margin[diff])
        assert anc.min() >= 0 and anc.max() < m
    # the fused form (weights in the advance launch) gives the same log-weights as the stand-alone entry on the same states
    chain = lorenz.make_chain()
    o = ops.chain_obs(index, shift, scale, 0.25, (chains.AffineObservation(index, shift, scale)(x[0]) + 0.1).float().contiguous())
    lw2, pm2, nxt = torch.empty(m, device=dev), torch.empty(len(pmax), device=dev), torch.empty(m, 3, device=dev)
    ops.chain_advance(chain.model(), x, nxt, 2, seed=SEED, obs=o, logw=lw2, pmax=pm2)
    lw3, pm3 = ops.bpf_logweights(nxt, o)
    assert torch.equal(lw2, lw3) and torch.equal(pm2, pm3)
    assert torch.equal(pm3, torch.stack([c.max() for c in lw3.split(256)]))


def test_weights_degenerate_cases(dev):
    # one particle holds all the weight: the others underflow to exactly 0
    x = torch.tensor([[4.0, 0.0, 25.0]] + [[4.0 + 3.0 * (i + 1), 0.0, 25.0] for i in range(64)])
    x, logw, pmax, ref = _weights_case(dev, 65, [0], [0.0], [8.0], 0.01, x=x, y=torch.tensor([0.5]))
    w, cdf, status = ops.bpf_cdf(logw, pmax)
    assert w.cpu().tolist() == [1.0] + [0.0] * 64 and int(status) == 0
    assert (ops.bpf_resample(cdf, SEED, 0) == 0).all()
    # every log-weight -inf (states at infinity): the wrapper raises where torch.multinomial would, nothing divides by zero
    xinf = torch.full((300, 3), float('inf'), device=dev)
    o = ops.chain_obs([0], [0.0], [8.0], 0.25, torch.tensor([0.5], device=dev))
    lw, pm = ops.bpf_logweights(xinf, o)
    assert torch.isinf(lw).all() and (lw < 0).all()
    with pytest.raises(_lib.SdaHipError):
        ops.bpf_cdf(lw, pm)
    lw[7] = float('nan')
    with pytest.raises(_lib.SdaHipError):
        ops.bpf_cdf(lw, None)
    with pytest.raises(_lib.SdaHipError):
        lorenz.posterior(torch.full((2, 1), float('inf')), A=chains.AffineObservation([0], [0.0], [8.0]), sigma=0.25, particles=64,
                         device=dev, seed=1)
    with pytest.raises(_lib.SdaHipError):
        ops.bpf_logweights(xinf.cpu(), o)
    # ... and the process goes on
    w, cdf, status = ops.bpf_cdf(torch.zeros(300, device=dev))
    assert int(status) == 0 and torch.equal(cdf, torch.arange(1, 301, device=dev, dtype=torch.float64))


def test_resampling_frequencies(dev):
    """4096 draws from weights proportional to (1, 2, 3, 4) repeated: the four class counts within 5 binomial standard
    deviations of 4096 p (fixed seed: deterministic)."""
    m = 4096
    logw = torch.tensor([1.0, 2.0, 3.0, 4.0], device=dev).log().repeat(m // 4)
    _, cdf, _ = ops.bpf_cdf(logw)
    anc = ops.bpf_resample(cdf, SEED, 1).cpu().numpy()
    counts = np.bincount(anc % 4, minlength=4)
    p = np.arange(1, 5) / 10
    assert (np.abs(counts - m * p) <= 5 * np.sqrt(m * p * (1 - p))).all(), counts
    assert len(np.unique(anc)) > m // 3                               # i.i.d. draws over all of the vector, not a few slots


@pytest.mark.parametrize('m,n,step', [(1, 1, 1), (65, 5, 3), (1000, 4, 2)])
def test_traceback(dev, m, n, step):
    """The one-launch traceback equals the reference's literal cat / re-gather on the filter's own recorded states and ancestors."""
    g = U.golden()
    chain = lorenz.make_chain()
    torch.manual_seed(m)
    x = chain.trajectory(chain.prior((m,), device=dev), 8, last=True)
    y = torch.from_numpy(g['post/y'])[torch.arange(n) % 4].to(dev)
    rec = {}
    out = chains.bpf_fused(chain, x, y, chains.AffineObservation([0], [0.0], [8.0]), 1.0, step, seed=SEED, record=rec)
    S, anc = rec['S'].cpu().numpy(), rec['anc'].cpu().numpy()
    assert out.shape == (m, n * step + 1, 3)
    assert np.array_equal(out.cpu().numpy(), chain_ref.regather(S, anc, step))
    assert np.array_equal(S[0], x.cpu().numpy())
    if m > 1:
        assert any(len(np.unique(a)) < m for a in anc)               # (resampling did merge histories)


@pytest.fixture(scope='module')
def small_posterior(dev):
    g = U.golden()
    y = torch.from_numpy(g['post/y'])
    A = lambda x: chains.Lorenz63.preprocess(x)[..., :1]      # noqa: E731
    torch.manual_seed(2024)
    fused = lorenz.posterior(y, A=A, sigma=0.25, step=2, particles=2048, fused=True, device=dev)
    assert lorenz.LAST_POSTERIOR_ROUTE == 'fused'
    generic = lorenz.posterior(y, A=A, sigma=0.25, step=2, particles=2048, fused=False, device=dev)
    assert lorenz.LAST_POSTERIOR_ROUTE == 'generic'
    return g, y, A, fused, generic


def test_posterior_shapes_and_routes(dev, small_posterior):
    g, y, A, fused, generic = small_posterior
    assert fused.shape == generic.shape == (2048, 4 * 2 - 2 + 1, 3)
    assert torch.isfinite(fused).all() and torch.isfinite(generic).all()
    with pytest.raises(_lib.SdaHipError):
        lorenz.posterior(y, A=lambda x: x[..., :1] ** 2, sigma=0.25, step=2, particles=64, fused=True, device=dev)
    lorenz.posterior(y, A=lambda x: x[..., :1] ** 2, sigma=4.0, step=2, particles=64, device=dev)
    assert lorenz.LAST_POSTERIOR_ROUTE == 'generic'                   # 'auto' with an operator that is not affine


def test_posterior_against_reference_samples(dev, small_posterior):
    """The first 256 device samples against reference set A: earth mover's distance (the oracle's exact LP) at most 1.25 x the
    largest of the eight reference-versus-reference distances in the fixture.  And the posterior explains y better than
    unconditioned trajectories do."""
    from oracle import sda_oracle as O
    g, y, A, fused, generic = small_posterior
    ref_a = torch.from_numpy(g['post/A'])
    limit = 1.25 * g['post/emd_ref'].max()
    d_fused = float(O.emd(fused[:256].cpu(), ref_a))
    d_generic = float(O.emd(generic[:256].cpu(), ref_a))
    print(f'emd fused {d_fused:.4f} generic {d_generic:.4f} reference pairs {np.round(g["post/emd_ref"], 4).tolist()} limit {limit:.4f}')
    assert d_fused <= limit
    assert d_generic <= limit
    chain = lorenz.make_chain()
    torch.manual_seed(7)
    free = chain.trajectory(chain.trajectory(chain.prior((256,), device=dev), 64, last=True), 7).transpose(0, 1)
    yd = y.to(dev)
    ll_post = lorenz.log_likelihood(yd, fused[:256], A=A, sigma=0.25, step=2).mean()
    ll_free = lorenz.log_likelihood(yd, free, A=A, sigma=0.25, step=2).mean()
    assert ll_post > ll_free


DRIVER = ('from sda.mcs import *\nfrom sda.score import *\nfrom sda.utils import *\n'
          'from sda_amd.experiments.lorenz import *\n')
SCRIPT = '''import sys
sys.path.insert(0, {root!r})
import sda_amd
sda_amd.install_as_sda(native_chains=True)
sys.path.insert(0, 'experiments/lorenz')
from utils import *
import sda_amd.experiments.lorenz as L
chain = make_chain()
torch.manual_seed(0)
x = chain.trajectory(chain.trajectory(chain.prior((), device='cuda'), 64, last=True), 7)
y = torch.normal(chain.preprocess(x[::2])[..., :1], 0.25)
xs = posterior(y, A=lambda x: chain.preprocess(x)[..., :1], sigma=0.25, step=2, particles=512)
lp = log_prior(xs)
ll = log_likelihood(y, xs, A=lambda x: chain.preprocess(x)[..., :1], sigma=0.25, step=2)
assert torch.isfinite(xs).all() and torch.isfinite(lp).all() and torch.isfinite(ll).all()
print('DROPIN', type(chain).__module__, L.LAST_POSTERIOR_ROUTE, tuple(xs.shape), tuple(lp.shape), tuple(ll.shape))
'''


def test_dropin_driver_with_native_chains(dev, tmp_path):
    """A stand-in driver file (the reference's star imports) in a fresh child process: make_chain / posterior / log_prior /
    log_likelihood run through the fused route, reached by the probe from the reference's own lambda."""
    (tmp_path / 'experiments' / 'lorenz').mkdir(parents=True)
    (tmp_path / 'experiments' / 'lorenz' / 'utils.py').write_text(DRIVER)
    out = subprocess.run([sys.executable, '-B', '-c', SCRIPT.format(root=ROOT)], cwd=tmp_path, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('DROPIN')][0]
    assert line == "DROPIN sda_amd.chains fused (512, 7, 3) (512,) (512,)"
