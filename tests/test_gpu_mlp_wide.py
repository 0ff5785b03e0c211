"""GPU: the whole-MLP kernels at widths up to 256 (csrc/mlp1d.hip, the _wide kernels: a GEMM streamed through LDS as 128 x 128 units) --
the width of the reference's trained Lorenz local nets (experiments/lorenz/train.py:30-44: LOCAL_CONFIG, width 256, depth 5).  Same
comparisons and tolerances as tests/test_gpu_net.py::test_whole_mlp_kernel_equals_layer_path_and_oracle and tests/test_gpu_fused1d.py
apply to the 128 kernels: per-layer kernels 1e-5, float64 oracle 1e-4, six PC steps against the general path 5e-5, graph replay 1e-6."""
import ctypes
import json

import pytest
import torch

from oracle import sda_oracle as O
from tests.util import assert_close, oracle_eps_from_module

pytestmark = pytest.mark.gpu
TOL = 1e-4
WIDTH = 256


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.mark.parametrize('rows,widths,act', [(61, (256,) * 5, 'SiLU'), (40000, (256,) * 5, 'SiLU'), (33000, (64, 256, 128), 'GELU'),
                                              (1000, (130,), 'ELU'), (7, (192, 256, 144), 'ReLU'), (4097, (200,) * 2, 'SELU')])
def test_wide_mlp_kernel_equals_layer_path_and_oracle(dev, rows, widths, act, monkeypatch):
    """Forward and input VJP of a whole ResMLP with GEMMs wider than 128 against the per-layer kernels and the float64 oracle: the
    reference's local net (47 -> 5 x 256 -> 15) on a short and a long batch, narrow <-> wide transitions in both directions, ragged widths
    on both sides of 128, every activation family, ragged last tiles."""
    from sda_amd import mlp
    from sda_amd.nn import ResMLP
    from sda_amd.utils import ACTIVATIONS
    torch.manual_seed(rows % 1000)
    in_f, out_f = 47, 15
    net = ResMLP(in_f, out_f, hidden_features=list(widths), activation=ACTIVATIONS[act]).to(dev)
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    cfg = O.ResMLPConfig(in_f, out_f, tuple(widths), act)
    x = torch.randn(rows, in_f)
    g = torch.randn(rows, out_f)
    sl = slice(max(0, rows - 50), rows)
    xo = x[sl].double().requires_grad_(True)
    ro = O.resmlp_forward(sd, '', cfg, xo)
    gref, = torch.autograd.grad(ro, xo, g[sl].double())

    def run(fused):
        monkeypatch.setattr(mlp, 'FUSED', fused)
        xd = x.to(dev).requires_grad_(True)
        out = net(xd)
        gx, = torch.autograd.grad(out, xd, g.to(dev))
        return out.detach(), gx
    out_f_, gx_f = run(True)
    out_l, gx_l = run(False)
    monkeypatch.setattr(mlp, 'FUSED', True)
    assert mlp._fused_plan(list(net)) is not None, 'the whole-MLP planner declined a net of width <= 256'
    assert_close(out_f_.cpu(), out_l.cpu(), 1e-5, what='fused vs per-layer forward')
    assert_close(gx_f.cpu(), gx_l.cpu(), 1e-5, what='fused vs per-layer VJP')
    assert_close(out_f_[sl].cpu(), ro.detach(), TOL, what='fused forward vs fp64 oracle')
    assert_close(gx_f[sl].cpu(), gref, TOL, what='fused VJP vs fp64 oracle')
    with torch.no_grad():
        assert torch.equal(net(x.to(dev)), out_f_)                  # the no-grad call (no saves) is bitwise the saving forward


def _build_local(dev, features, window, affine, seed=90, width=WIDTH):
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


LOCAL_CASES = [
    # B, L, C, window, slices, per-sample y, affine  (the shapes of tests/test_gpu_fused1d.py::LOCAL_CASES)
    (5, 65, 3, 5, (slice(None, None, 8), slice(0, 1)), False, True),
    (1100, 65, 3, 5, (slice(None, None, 1), slice(0, 1)), False, False),
    (9, 17, 3, 5, (slice(3, 15, 5), slice(1, 3)), True, False),
    (1, 5, 3, 5, (slice(0, None, 2),), False, True),
    (70, 30, 5, 3, (slice(None, None, 4), slice(0, 5, 2)), True, True),
    (33, 12, 2, 5, (slice(None, None, 3), slice(0, 1)), True, False),
]


@pytest.mark.parametrize('case', LOCAL_CASES)
def test_fused_local_evaluation_at_width_256(dev, case, monkeypatch):
    """The guided evaluation of a width-256 local net takes the three-launch route (sda_mlp_fwd_win, sda_mlp_bwd_win, sda_mc_finish) and
    agrees with the general path and the oracle."""
    from sda_amd import fused1d, observe as Ob
    from sda_amd.score import GaussianScore
    B, L, C, window, sl, per_sample, affine = case
    net, inner = _build_local(dev, C, window, affine)
    torch.manual_seed(91)
    x = torch.randn(B, L, C)
    t = torch.tensor(0.41)
    A = Ob.Subsample(sl)
    oshape = A._osize(x.shape)
    y = torch.randn(oshape if per_sample else oshape[1:])
    gs = GaussianScore(y, A=A, std=0.3, sde=inner, gamma=3e-2).to(dev)
    xd, td = x.to(dev), t.to(dev)
    fz = fused1d.plan(gs, xd, td, None)
    assert isinstance(fz, fused1d.FusedLocal), 'the fused plan declined a width-256 local net'
    got = gs(xd, td)
    assert torch.equal(got, gs(xd, td))
    monkeypatch.setattr(fused1d, 'ENABLED', False)
    ref = gs(xd, td)
    monkeypatch.setattr(fused1d, 'ENABLED', True)
    assert_close(got.cpu(), ref.cpu(), 1e-5, what='fused vs general path (wide local net)')
    eps_net = oracle_eps_from_module(net, 'local')
    sched = O.Schedule()

    def eps_o(xx, tt):
        if not affine:
            return eps_net(xx, tt)
        mu, sg = sched.mu(tt), sched.sigma(tt)
        return xx * (sg / (mu * mu + sg * sg)) + 0.1 * eps_net(xx, tt)
    rows = slice(max(0, B - 6), B)
    Af = lambda v: v[(Ellipsis,) + tuple(sl)]
    ref_o = O.gaussian_score(eps_o, sched, y[rows] if per_sample else y, Af, 0.3, 3e-2, x[rows], t)
    assert_close(got[rows].cpu(), ref_o, TOL, what='fused vs oracle (wide local net)')


@pytest.mark.parametrize('B,L,corr,noise', [(300, 65, 2, 'keyed'), (300, 65, 2, 'torch'), (1, 65, 1, 'keyed'), (40, 9, 0, 'torch')])
def test_fused_local_pc_steps_at_width_256_eager_and_graph(dev, B, L, corr, noise, monkeypatch):
    from sda_amd import fused1d, observe as Ob, parallel
    from sda_amd.score import GaussianScore, VPSDE
    C = 3
    net, inner = _build_local(dev, C, 5, True, seed=92)
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
    assert_close(fe.cpu(), base.cpu(), 5e-5, what='6 fused steps vs the general path (wide local net)')
    fg = run(True, True)
    assert_close(fg.cpu(), fe.cpu(), 1e-6, what='fused graph replay vs fused eager (wide local net)')
    monkeypatch.setattr(fused1d, 'ENABLED', True)


def test_reference_local_checkpoint_round_trip_takes_the_fused_route(dev, tmp_path):
    """state.pth + config.json as the reference's train_local writes them (experiments/lorenz/train.py:30-44, 88-91), with LOCAL_CONFIG's own
    values.  The weights are a random initialisation -- no trained checkpoint ships with the sources; what is checked is that a net of that
    configuration loads, takes the fused guided evaluation and agrees with the general path."""
    from sda_amd import fused1d, observe as Ob
    from sda_amd.experiments.lorenz import load_score, make_local_score
    from sda_amd.score import GaussianScore, VPSDE
    config = {'window': 5, 'embedding': 32, 'width': 256, 'depth': 5, 'activation': 'SiLU', 'epochs': 4096, 'batch_size': 64,
              'optimizer': 'AdamW', 'learning_rate': 1e-3, 'weight_decay': 1e-3, 'scheduler': 'linear'}
    torch.manual_seed(95)
    src = make_local_score(**config)
    torch.save(src.state_dict(), tmp_path / 'state.pth')
    (tmp_path / 'config.json').write_text(json.dumps(config))
    score = load_score(tmp_path / 'state.pth', local=True)
    widths = {l.out_features for l in score.kernel.network.modules() if isinstance(l, torch.nn.Linear)}
    assert max(widths) == 256
    for a, b in zip(src.state_dict().values(), score.state_dict().values()):
        assert torch.equal(a, b)
    score = score.to(dev)
    x = torch.randn(8, 65, 3, device=dev)
    t = torch.tensor(0.3, device=dev)
    A = Ob.Subsample((slice(None, None, 8), slice(0, 1)))
    y = torch.randn(A._osize(x.shape)[1:])
    gs = GaussianScore(y, A=A, std=0.05, sde=VPSDE(score, shape=()), gamma=1e-2).to(dev)
    assert isinstance(fused1d.plan(gs, x, t, None), fused1d.FusedLocal)
    got = gs(x, t)
    fused1d.ENABLED = False
    try:
        ref = gs(x, t)
    finally:
        fused1d.ENABLED = True
    assert_close(got.cpu(), ref.cpu(), 1e-5, what='loaded width-256 checkpoint: fused vs general path')


def test_narrow_net_is_unchanged_next_to_the_wide_kernels(dev, monkeypatch):
    """A width-128 net still runs the narrow kernels: bitwise repeatable, and equal to the per-layer route at 1e-5."""
    from sda_amd import mlp
    from sda_amd.nn import ResMLP
    from sda_amd.utils import ACTIVATIONS
    torch.manual_seed(5)
    net = ResMLP(47, 15, hidden_features=[128] * 5, activation=ACTIVATIONS['SiLU']).to(dev)
    x = torch.randn(5000, 47, device=dev)
    g = torch.randn(5000, 15, device=dev)

    def run(fused):
        monkeypatch.setattr(mlp, 'FUSED', fused)
        xd = x.clone().requires_grad_(True)
        out = net(xd)
        gx, = torch.autograd.grad(out, xd, g)
        return out.detach(), gx
    o1, g1 = run(True)
    o2, g2 = run(True)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    ol, gl = run(False)
    assert_close(o1.cpu(), ol.cpu(), 1e-5, what='width 128: fused vs per-layer forward')
    assert_close(g1.cpu(), gl.cpu(), 1e-5, what='width 128: fused vs per-layer VJP')


def test_c_abi_accepts_256_and_refuses_257(dev):
    """sda_mlp_fwd called directly: one Linear 256 -> 256 runs (and computes W x + b); 257 is SDA_E_UNSUPPORTED and launches nothing."""
    from sda_amd import _lib, mlp, ops
    lib = _lib.load()
    torch.manual_seed(6)
    rows = 100
    W = torch.randn(256, 256, device=dev) / 16
    b = torch.randn(256, device=dev)
    x = torch.randn(rows, 256, device=dev)
    out = torch.full((rows, 256), 7.0, device=dev)
    slab = mlp._slab(W)
    assert slab.numel() == lib.sda_mlp_slab_floats(256, 256)

    def desc(width):
        d = _lib.MlpDesc()
        d.rows, d.ngemm, d.act, d.unbiased, d.eps = rows, 1, 0, 0, 1e-5
        d.kind[0], d.in_f[0], d.out_f[0], d.w_off[0], d.b_off[0] = 0, width, width, 0, 0
        d.w, d.bias = slab.data_ptr(), b.data_ptr()
        d.x, d.x_ld, d.out, d.out_ld = x.data_ptr(), 256, out.data_ptr(), 256
        return d
    assert lib.sda_mlp_fwd(ctypes.byref(desc(257)), ops._stream()) == -2  # SDA_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'a refused descriptor wrote to the output'
    assert lib.sda_mlp_fwd(ctypes.byref(desc(256)), ops._stream()) == 0  # SDA_OK
    torch.cuda.synchronize()
    ref = x.double() @ W.double().t() + b.double()
    assert_close(out.cpu(), ref.cpu(), TOL, what='sda_mlp_fwd 256 -> 256 vs float64')
