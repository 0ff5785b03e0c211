"""GPU: the fused guided evaluation of a LOCAL score network (sda_amd/fused1d.py: FusedLocal -- sda_mlp_fwd_win, sda_mlp_bwd_win,
sda_mc_finish) at windows of 17 .. 32 values, i.e. two D fragments per row: the k = 3 and k = 4 checkpoints of experiments/lorenz/eval.py:32-38
(windows of 7 and 9 states of 3 values).  Against the general path (unfold + cat + whole-MLP kernels + fold + the guidance kernels) and the
oracle, with the bounds tests/test_gpu_fused1d.py holds this route to at windows 3 and 5."""
import pytest
import torch

from oracle import sda_oracle as O
from tests.util import assert_close, oracle_eps_from_module

pytestmark = pytest.mark.gpu
TOL = 1e-4                  # (tests/test_gpu_fused1d.py: TOL)


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _build_local(dev, features, window, affine, seed=90, width=128):
    # (tests/test_gpu_fused1d.py: _build_local)
    import bench
    from sda_amd.experiments.lorenz import make_local_score
    from sda_amd.score import VPSDE
    torch.manual_seed(seed)
    net = make_local_score(window=window, features=features, width=width).to(dev)
    if affine:
        score = bench.SyntheticScore(net)
        inner = VPSDE(score, shape=())
        object.__setattr__(score, '_sched', inner)
    else:
        inner = VPSDE(net, shape=())
    return net, inner


def _oracle_eps(net, affine, width):
    eps_net = oracle_eps_from_module(net, 'local', hidden=(width,) * 5)
    sched = O.Schedule()

    def eps_o(xx, tt, dtype=None):
        e = eps_net(xx, tt) if dtype is None else eps_net(xx, tt, dtype=dtype)
        if not affine:
            return e
        mu, sg = sched.mu(tt), sched.sigma(tt)
        return xx * (sg / (mu * mu + sg * sg)) + 0.1 * e
    return eps_o, sched


def _close_or_no_worse(got, ref, rtol, what, ref64):
    """`got` within rtol of `ref` (assert_close); where rounding alone puts it outside -- the overlap sum has up to 9 terms at these windows --
    both are measured against the float64 oracle instead and `got` must be no further from it than `ref` is."""
    try:
        assert_close(got, ref, rtol, what=what)
    except AssertionError as exc:
        r64 = ref64()
        e_got = (got.double().cpu() - r64).abs().max().item()
        e_ref = (ref.double().cpu() - r64).abs().max().item()
        print(f'{what}: {exc}; against the float64 oracle: fused {e_got:.3e}, general path {e_ref:.3e}')
        assert e_got <= e_ref, f'{what}: {exc}; error against the float64 oracle {e_got:.3e} (fused) > {e_ref:.3e} (general path)'


CASES = [
    # B, L, C, window, slices, per-sample y, affine, width
    (5, 65, 3, 7, (slice(None, None, 8), slice(0, 1)), False, True, 128),       # eval.py "lo" at k = 3
    (5, 65, 3, 9, (slice(None, None, 1), slice(0, 1)), False, False, 128),      # eval.py "hi" at k = 4, bare network
    (3, 9, 3, 9, (slice(0, None, 2),), False, True, 128),                        # one window per trajectory: first and last at once
    (4, 10, 3, 9, (slice(3, 9, 5), slice(1, 3)), True, False, 128),              # two windows, both edge windows; offsets and stops
    (9, 20, 2, 9, (slice(None, None, 3), slice(0, 1)), True, False, 128),        # wc = 18: just over one fragment
    (7, 12, 6, 5, (slice(None, None, 4), slice(0, 6, 2)), True, True, 128),      # wc = 30: fragment 1 nearly full, channel stride
    (11, 17, 3, 9, (slice(None, None, 4), slice(0, 2)), True, False, 100),       # the masked LayerNorm width; 99 rows: a partial last tile
    (5, 33, 3, 7, (slice(None, None, 8), slice(0, 1)), False, True, 256),        # the wide kernels, k = 3
    (5, 33, 3, 9, (slice(None, None, 1), slice(0, 1)), False, False, 256),       # the wide kernels, k = 4
]


@pytest.mark.parametrize('case', CASES)
def test_fused_local_evaluation_window32_equals_general_path_and_oracle(dev, case, monkeypatch):
    from sda_amd import fused1d, observe as Ob
    from sda_amd.score import GaussianScore
    B, L, C, window, sl, per_sample, affine, width = case
    assert 16 < window * C <= 32
    net, inner = _build_local(dev, C, window, affine, width=width)
    torch.manual_seed(91)
    x = torch.randn(B, L, C)
    t = torch.tensor(0.41)
    A = Ob.Subsample(sl)
    oshape = A._osize(x.shape)
    y = torch.randn(oshape if per_sample else oshape[1:])
    gs = GaussianScore(y, A=A, std=0.3, sde=inner, gamma=3e-2).to(dev)
    xd, td = x.to(dev), t.to(dev)
    fz = fused1d.plan(gs, xd, td, None)
    assert isinstance(fz, fused1d.FusedLocal), f'the fused plan declined a local net with a window of {window * C} values'
    assert fz.gwin.shape == (B * (L - window + 1), 32)
    got = gs(xd, td)
    assert torch.equal(got, gs(xd, td))
    monkeypatch.setattr(fused1d, 'ENABLED', False)
    ref = gs(xd, td)
    monkeypatch.setattr(fused1d, 'ENABLED', True)
    eps_o, sched = _oracle_eps(net, affine, width)
    Af = lambda v: v[(Ellipsis,) + tuple(sl)]

    def ref64():
        return O.gaussian_score(lambda xx, tt: eps_o(xx, tt, dtype=torch.float64), sched, y.double(), Af, 0.3, 3e-2, x.double(), t.double())
    _close_or_no_worse(got.cpu(), ref.cpu(), 1e-5, 'fused vs general path (local net, two-fragment window)', ref64)
    rows = slice(max(0, B - 6), B)
    ref_o = O.gaussian_score(eps_o, sched, y[rows] if per_sample else y, Af, 0.3, 3e-2, x[rows], t)
    assert_close(got[rows].cpu(), ref_o, TOL, what='fused vs oracle (local net, two-fragment window)')


@pytest.mark.parametrize('B,L,corr', [(1, 65, 1), (70, 33, 2)])
@pytest.mark.parametrize('noise', ['keyed', 'torch'])
@pytest.mark.parametrize('window', [7, 9])
def test_fused_local_pc_steps_window32_equal_general_path_eager_and_graph(dev, window, B, L, corr, noise, monkeypatch):
    from sda_amd import fused1d, observe as Ob, parallel
    from sda_amd.score import GaussianScore, VPSDE
    C = 3
    net, inner = _build_local(dev, C, window, True, seed=92)
    torch.manual_seed(93)
    x1 = torch.randn(B, L, C)
    A = Ob.Subsample((slice(None, None, 8), slice(0, 1)))
    y = torch.randn(A._osize(x1.shape)[1:])
    gs = GaussianScore(y, A=A, std=0.2, sde=inner, gamma=3e-2)
    sde = VPSDE(gs, shape=(L, C)).to(dev)

    def run(fused, graph):
        monkeypatch.setattr(fused1d, 'ENABLED', fused)
        sde.initial_noise = x1
        sde.noise_source = parallel.KeyedNoise((5, 5 + B), (L, C), 9, corr, dev) if noise == 'keyed' and corr else None
        torch.manual_seed(94)
        sampler = sde.sampler((B,), steps=50, corrections=corr, tau=0.25)
        assert isinstance(sampler._fused, fused1d.FusedLocal) == fused
        if graph:
            sampler.capture()
        for _ in range(6):
            sampler.step()
        torch.cuda.synchronize()
        sde.initial_noise, sde.noise_source = None, None
        return sampler.result().clone()

    base = run(False, False)
    assert torch.isfinite(base).all()
    fe = run(True, False)
    assert_close(fe.cpu(), base.cpu(), 5e-5, what='6 fused steps vs the general path (local net, two-fragment window)')
    fg = run(True, True)
    assert_close(fg.cpu(), fe.cpu(), 1e-6, what='fused graph replay vs fused eager (local net, two-fragment window)')
    monkeypatch.setattr(fused1d, 'ENABLED', True)


@pytest.mark.parametrize('C,window', [(3, 11), (11, 3)])
def test_windows_above_32_values_take_the_general_path(dev, C, window):
    from sda_amd import fused1d, observe as Ob
    from sda_amd.score import GaussianScore
    assert window * C == 33
    B, L = 4, 14
    net, inner = _build_local(dev, C, window, False)
    torch.manual_seed(95)
    x = torch.randn(B, L, C)
    t = torch.tensor(0.41)
    sl = (slice(None, None, 3), slice(0, 1))
    A = Ob.Subsample(sl)
    y = torch.randn(A._osize(x.shape)[1:])
    gs = GaussianScore(y, A=A, std=0.3, sde=inner, gamma=3e-2).to(dev)
    xd, td = x.to(dev), t.to(dev)
    assert not isinstance(fused1d.plan(gs, xd, td, None), fused1d.FusedLocal)
    eps_o, sched = _oracle_eps(net, False, 128)
    ref_o = O.gaussian_score(eps_o, sched, y, lambda v: v[(Ellipsis,) + tuple(sl)], 0.3, 3e-2, x, t)
    assert_close(gs(xd, td).cpu(), ref_o, TOL, what='general path vs oracle (window of 33 values)')


@pytest.mark.parametrize('window,stride', [(5, 16), (7, 32)])
def test_gwin_row_stride_follows_the_window(dev, window, stride):
    from sda_amd import fused1d, observe as Ob
    from sda_amd.score import GaussianScore
    B, L, C = 2, 12, 3
    net, inner = _build_local(dev, C, window, False)
    x = torch.zeros(B, L, C, device=dev)
    A = Ob.Subsample((slice(None, None, 2), slice(0, 1)))
    gs = GaussianScore(torch.zeros(A._osize(x.shape)[1:]), A=A, std=0.3, sde=inner, gamma=3e-2).to(dev)
    fz = fused1d.plan(gs, x, torch.tensor(0.5, device=dev), None)
    assert isinstance(fz, fused1d.FusedLocal)
    assert fz.gwin.shape == (B * (L - window + 1), stride)


def test_fused_forward_epilogue_window32_is_the_unfused_guidance_kernel_bit_for_bit(dev):
    """The two-fragment windows' epilogue (csrc/guide.hpp through ml_win_fold<2>): ghat == sda_obs_subsample_guidance on the eps it wrote."""
    from sda_amd import fused1d, observe as Ob
    from sda_amd.score import GaussianScore
    B, L, C, window, sl, per_sample, affine, width = CASES[3]                 # two windows, both edge windows; offsets and stops
    net, inner = _build_local(dev, C, window, affine, width=width)
    torch.manual_seed(91)
    x = torch.randn(B, L, C, device=dev)
    t = torch.tensor(0.41, device=dev)
    A = Ob.Subsample(sl)
    gs = GaussianScore(torch.randn(A._osize(x.shape)), A=A, std=0.3, sde=inner, gamma=3e-2).to(dev)
    fz = fused1d.plan(gs, x, t, None)
    assert isinstance(fz, fused1d.FusedLocal) and fz.gwin.shape[1] == 32
    fz.prologue_eval(t)
    fz.forward(x, 0)
    ref = A.gaussian_guidance(x, fz.eps, gs.y, 0.3, 3e-2, fz.coef[0], fz.coef[1])       # (adjacent 0-dim views: travels as coef_dev)
    assert ref is not None and ref.abs().sum().item() > 0
    assert torch.equal(fz.ghat, ref)
