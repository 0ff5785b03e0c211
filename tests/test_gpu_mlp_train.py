"""GPU: opt-in parameter gradients of ScoreNet / ResMLP (sda_amd.training with mlp = True; csrc/mlp_train.hip).

Kernel level: the cotangent streams of sda_mlp_bwd_train and the batched weight gradient sda_mlp_wgrad against float64 torch.autograd.
Whole net: the gradients of ``VPSDE.loss(x, w).backward()`` against torch.autograd of the oracle's float64 ``score_net`` on the same
t / eps draws; bitwise repeatability, accumulation, an SGD trajectory against the oracle, ``utils.loop`` and the untouched sampling VJP."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import sda_oracle as O
from sda_amd import _lib, mlp, ops, training
from sda_amd._lib import load as load_lib
from sda_amd.nn import ResMLP
from sda_amd.score import MCScoreNet, ScoreNet, VPSDE
from tests import mlp_train_ref as R
from tests.util import load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _tiny(dev):
    """The ``scorenet_local_tiny`` golden net: MCScoreNet(3, order=2) over ScoreNet(15, embedding=8, 16 x 2, SiLU)."""
    _, grp = load_golden('scorenet_local_tiny')
    net = MCScoreNet(features=3, order=2, embedding=8, hidden_features=[16] * 2, activation=nn.SiLU)
    net.load_state_dict(grp['sd'])
    return net.to(dev), O.ResMLPConfig(15 + 8, 15, (16, 16), 'SiLU')


# ------------------------------------------------------------------------------------------------------------ sda_mlp_bwd_train

class _Ctx:
    """Stands in for the autograd context of _TrainMLPFunction.forward: keeps what it saves."""

    def save_for_backward(self, sv, stats, *inputs):
        self.sv, self.stats, self.inputs = sv, stats, inputs


def _streams(net, x, g):
    """The training forward (segments, saves) of ResMLP ``net`` on rows ``x``, then sda_mlp_bwd_train and sda_mlp_bwd on the SAME descriptor:
    (input gradient of each, g_save [gemm][rows][g_ld] NaN-filled with a padded g_ld, the plan)."""
    plan = mlp._fused_plan(list(net))
    ctx = _Ctx()
    with torch.no_grad():
        mlp._TrainMLPFunction.forward(ctx, x, plan)
    rows, ld, g_ld = x.shape[0], plan.save_ld, plan.g_ld + 8
    t = _lib.MlpTrainDesc()
    d = plan.desc(rows, True, d=t.mlp)
    gx = torch.full((rows, plan.gemms[0][1]), float('nan'), device=x.device)
    gx0 = torch.full_like(gx, float('nan'))
    g_save = torch.full((len(plan.gemms), rows, g_ld), float('nan'), device=x.device)
    d.x, d.x_ld, d.out, d.out_ld = g.data_ptr(), g.stride(0), gx.data_ptr(), gx.stride(0)
    d.a_save, d.z_save, d.save_stride, d.save_ld = ctx.sv[0].data_ptr(), ctx.sv[1].data_ptr(), rows * ld, ld
    d.mean_save, d.rstd_save, d.stat_stride = ctx.stats[0].data_ptr(), ctx.stats[1].data_ptr(), rows
    t.g_save, t.g_stride, t.g_ld = g_save.data_ptr(), rows * g_ld, g_ld
    ops.mlp_bwd_train(t)
    d0 = _lib.MlpDesc.from_buffer_copy(t.mlp)
    d0.out = gx0.data_ptr()
    ops.mlp_launch(d0, True)
    torch.cuda.synchronize()
    return gx, gx0, g_save, plan


def _cotangents64(net, cfg, x, g):
    """float64 autograd of the oracle's resmlp_forward: the cotangent at a GEMM's output is the gradient of that GEMM's bias, taken per
    row (the bias expanded to one copy per row) -> (input gradient, [per GEMM: [rows][out_f]])."""
    rows = x.shape[0]
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    biases = [k for k in sd if k.endswith('bias')]
    for k in biases:
        sd[k] = sd[k].expand(rows, -1).clone().requires_grad_(True)
    x64 = x.double().cpu().requires_grad_(True)
    out = O.resmlp_forward(sd, '', cfg, x64)
    grads = torch.autograd.grad((out * g.double().cpu()).sum(), [x64] + [sd[k] for k in biases])
    return grads[0], list(grads[1:])


STREAM_NETS = {
    'tiny': lambda: (None, None),
    '47-128x3-15': lambda: (ResMLP(15 + 32, 15, hidden_features=(128,) * 3, activation=nn.SiLU), O.ResMLPConfig(47, 15, (128,) * 3, 'SiLU')),
    '47-256x5-15': lambda: (ResMLP(47, 15, hidden_features=(256,) * 5, activation=nn.SiLU), O.ResMLPConfig(47, 15, (256,) * 5, 'SiLU')),
}


@pytest.mark.parametrize('name', list(STREAM_NETS))
def test_bwd_train_streams_match_float64(dev, name):
    torch.manual_seed(1)
    net, cfg = STREAM_NETS[name]()
    if net is None:
        mc, cfg = _tiny(dev)
        net = mc.kernel.network
    net = net.to(dev)
    for rows in (1, 16, 17, 64, 65, 1000):
        x = torch.randn(rows, cfg.in_features, device=dev)
        g = torch.randn(rows, cfg.out_features, device=dev)
        gx, gx0, g_save, plan = _streams(net, x, g)
        assert torch.equal(gx, gx0), rows                     # (the helpers are shared: the input gradient is sda_mlp_bwd's, bitwise)
        gx64, cots = _cotangents64(net, cfg, x, g)
        assert rel_err(gx, gx64) <= 1e-5, (rows, rel_err(gx, gx64))
        assert len(cots) == len(plan.gemms)
        for j, (ref, (_k, _i, o, _lin)) in enumerate(zip(cots, plan.gemms)):
            got = g_save[j, :, :o]
            err = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
            assert err <= 1e-5, (rows, j, err)
            pad = 16 if o <= 16 else (128 if o <= 128 else 256)
            assert (g_save[j, :, o:pad] == 0).all() and torch.isnan(g_save[j, :, pad:]).all(), (rows, j)


# ------------------------------------------------------------------------------------------------------------ sda_mlp_wgrad

def _device_run(lib):
    def run(d):
        assert lib.sda_mlp_wgrad(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
    return run


# the host grid thinned: per kind every rows value and every shape at least once
WGRAD_CASES = [(rows, R.SHAPES[(i + kind) % len(R.SHAPES)], kind) for kind in R.KINDS for i, rows in enumerate(R.ROWS)]


def test_wgrad_grid_is_covering():
    for kind in R.KINDS:
        assert {r for r, _s, k in WGRAD_CASES if k == kind} == set(R.ROWS)
        assert {s for _r, s, k in WGRAD_CASES if k == kind} == set(R.SHAPES)


@pytest.mark.parametrize('rows,shape,kind', WGRAD_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wgrad_matches_float64(dev, rows, shape, kind):
    lib = load_lib()
    R.check_case(_device_run(lib), lib, R.make_case(rows, shape[0], shape[1], kind, dev), dev)


@pytest.mark.parametrize('kind', R.KINDS)
def test_wgrad_4096_rows_several_slabs(dev, kind):
    lib = load_lib()
    case = R.make_case(4096, 256, 256, kind, dev)
    assert lib.sda_mlp_wgrad_slabs(ctypes.byref(R.wgrad_desc([case], R.buffers([case], dev)))) > 1      # (the planner's own choice)
    R.check_case(_device_run(lib), lib, case, dev)


@pytest.mark.parametrize('act', ['SiLU', 'GELU', 'ELU'])
def test_wgrad_activations(dev, act):
    lib = load_lib()
    R.check_case(_device_run(lib), lib, R.make_case(65, 17, 129, 2, dev, act=act), dev)


# ------------------------------------------------------------------------------------------------------------ whole nets

def _oracle_grads(module, eps_fn, x, t, e, weight):
    """float64 grads of the denoising loss through the oracle net over the module's state dict -> {name: grad}."""
    sd = {k: v.detach().double().cpu().requires_grad_(k in dict(module.named_parameters())) for k, v in module.state_dict().items()}
    sched = O.Schedule()
    t64, e64, x64 = t.double().cpu(), e.double().cpu(), x.double().cpu()
    tb = t64.reshape((-1,) + (1,) * (x.dim() - 1))
    xt = sched.mu(tb) * x64 + sched.sigma(tb) * e64
    err = (eps_fn(sd, xt, t64) - e64).square()
    loss = err.mean() if weight is None else (err * weight.double().cpu()).mean() / weight.double().cpu().mean()
    names = [k for k, p in module.named_parameters()]
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    return loss.detach(), dict(zip(names, grads))


def _hip_grads(module, shape, x, weight, seed, dev, zero=True):
    sde = VPSDE(module, shape=shape).to(dev)
    if zero:
        module.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    with training.parameter_gradients(mlp=True):
        loss = sde.loss(x, w=weight)
        loss.backward()
    torch.manual_seed(seed)
    t = torch.rand(x.shape[0], dtype=x.dtype, device=dev)
    e = torch.randn_like(x)
    return loss.detach(), {k: p.grad for k, p in module.named_parameters()}, t, e


def _check_net(module, shape, eps_fn, x, weight, dev, seed=11):
    loss, g, t, e = _hip_grads(module, shape, x, weight, seed, dev)
    loss64, g64 = _oracle_grads(module, eps_fn, x, t, e, weight)
    print(f'loss {loss.item():.8e} vs {loss64.item():.8e}')
    worst = {k: ((g[k].double().cpu() - ref).abs().max().item() / ref.abs().max().item() if g[k] is not None else None) for k, ref in g64.items()}
    print('max |grad - ref| / max |ref| per parameter:', {k: (None if v is None else f'{v:.2e}') for k, v in worst.items()})
    assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
    for k, ref in g64.items():
        got = g[k]
        assert got is not None, f'{k}: no gradient formed'
        err = (got.double().cpu() - ref).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, f'{k}: {err:.3e} vs scale {ref.abs().max().item():.3e}'
    assert any('embedding' in k for k in g64) and any('network' in k for k in g64)


def _scorenet_eps(cfg, prefix=''):
    return lambda sd, xt, t: O.score_net(sd, prefix, cfg, xt, t)


def _both_weights(module, shape, eps_fn, x, dev):
    torch.manual_seed(12)
    w = torch.rand(x.shape[:1] + (1,) * (x.dim() - 2) + x.shape[-1:], device=dev) + 0.5
    for weight in (None, w):
        _check_net(module, shape, eps_fn, x, weight, dev)


def test_net_gradients_tiny_kernel(dev):
    mc, cfg = _tiny(dev)
    torch.manual_seed(3)
    _both_weights(mc.kernel, (15,), _scorenet_eps(cfg), torch.randn(7, 15, device=dev), dev)


def test_net_gradients_local_config_64_rows(dev):
    """The reference's LOCAL_CONFIG kernel (window 5, embedding 32, width 256, depth 5, SiLU) at train_local's batch of 64 windows."""
    from sda_amd.experiments.lorenz import make_local_score
    torch.manual_seed(0)
    kernel = make_local_score(width=256, depth=5).kernel.to(dev)
    torch.manual_seed(4)
    _both_weights(kernel, (15,), _scorenet_eps(O.ResMLPConfig(47, 15, (256,) * 5, 'SiLU')), torch.randn(64, 15, device=dev), dev)


def test_net_gradients_default_local_65_rows(dev):
    from sda_amd.experiments.lorenz import make_local_score
    torch.manual_seed(1)
    kernel = make_local_score().kernel.to(dev)
    torch.manual_seed(5)
    _both_weights(kernel, (15,), _scorenet_eps(O.ResMLPConfig(47, 15, (128,) * 5, 'SiLU')), torch.randn(65, 15, device=dev), dev)


def test_net_gradients_linear_mid_chain(dev):
    torch.manual_seed(2)
    net = ScoreNet(15, embedding=32, hidden_features=(64, 128), activation=nn.SiLU).to(dev)
    torch.manual_seed(6)
    _both_weights(net, (15,), _scorenet_eps(O.ResMLPConfig(47, 15, (64, 128), 'SiLU')), torch.randn(33, 15, device=dev), dev)


def test_net_gradients_chain_that_starts_with_a_block(dev):
    """in_features + embedding == hidden_features[0]: no leading Linear, GEMM 0 is a block's, and the first segment's output (not the net
    input) is the operand of the first Linear's weight gradient."""
    torch.manual_seed(14)
    net = ScoreNet(3, embedding=13, hidden_features=(16, 16), activation=nn.SiLU).to(dev)
    plan = mlp._fused_plan(list(net.network))
    assert plan.gemms[0][0] == 1 and len(plan.segments) == 2
    torch.manual_seed(15)
    _both_weights(net, (3,), _scorenet_eps(O.ResMLPConfig(16, 3, (16, 16), 'SiLU')), torch.randn(19, 3, device=dev), dev)


def test_net_gradients_narrow_segment_in_a_wide_chain(dev):
    """hidden_features (256, 64): the 64-wide segment runs the narrow forward kernel, and the wide backward reads its saves."""
    torch.manual_seed(16)
    net = ScoreNet(15, embedding=32, hidden_features=(256, 64), activation=nn.SiLU).to(dev)
    torch.manual_seed(17)
    _both_weights(net, (15,), _scorenet_eps(O.ResMLPConfig(47, 15, (256, 64), 'SiLU')), torch.randn(33, 15, device=dev), dev)


def test_frozen_parameters_get_no_gradient_and_change_no_other(dev):
    """Linears whose weight and bias do not ask for a gradient drop out of the weight-gradient launch; the others' gradients are bitwise
    those of the all-trainable net."""
    mc, _ = _tiny(dev)
    kernel = mc.kernel
    torch.manual_seed(18)
    x = torch.randn(21, 15, device=dev)
    _, full, _, _ = _hip_grads(kernel, (15,), x, None, 22, dev)
    full = {k: v.clone() for k, v in full.items()}
    frozen = [k for k in full if k.startswith('network.1.')] + ['network.0.bias']      # a whole block; one half of a Linear
    for k, p in kernel.named_parameters():
        p.requires_grad_(k not in frozen)
    try:
        _, part, _, _ = _hip_grads(kernel, (15,), x, None, 22, dev)
    finally:
        for p in kernel.parameters():
            p.requires_grad_(True)
    assert len(frozen) == 5
    for k in full:
        if k in frozen:
            assert part[k] is None, k
        else:
            assert torch.equal(part[k], full[k]), k
    kernel.zero_grad(set_to_none=True)


def test_net_gradients_markov_chain_generic_route(dev):
    """A whole MCScoreNet(3, order=2) over the golden ScoreNet: unfold gather, ScoreNet on the window rows, fold.  ONE trajectory of 9
    steps: ScoreNet broadcasts the time embedding (B, E) against the windows (B, L - 2k, (2k + 1) C) by trailing axes, as the reference and
    the oracle do, so a per-sample t of ``VPSDE.loss`` fits a batch of one only (with B = 2 the reference's own broadcast raises)."""
    mc, cfg = _tiny(dev)

    def eps_fn(sd, xt, t):
        return O.mc_score_net(lambda a, b, c=None: O.score_net(sd, 'kernel.', cfg, a, b, c), 2, xt, t)
    with pytest.raises(RuntimeError):
        eps_fn({k: v.double().cpu() for k, v in mc.state_dict().items()}, torch.randn(2, 9, 3).double(), torch.rand(2).double())
    torch.manual_seed(7)
    _both_weights(mc, (9, 3), eps_fn, torch.randn(1, 9, 3, device=dev), dev)


@pytest.mark.parametrize('act', ['GELU', 'ELU'])
@pytest.mark.parametrize('unbiased', [True, False])
def test_net_gradients_activations_and_variance_conventions(dev, monkeypatch, act, unbiased):
    """Two more activations (SiLU is every net above), both LayerNorm variance conventions (the package's and the oracle's switches)."""
    import sda_amd.nn as snn
    monkeypatch.setattr(snn, 'LN_UNBIASED', unbiased)
    monkeypatch.setattr(O, 'LN_UNBIASED', unbiased)
    torch.manual_seed(8)
    net = ScoreNet(5, embedding=8, hidden_features=(24, 24), activation=getattr(nn, act)).to(dev)
    torch.manual_seed(9)
    _check_net(net, (5,), _scorenet_eps(O.ResMLPConfig(13, 5, (24, 24), act)), torch.randn(17, 5, device=dev), None, dev)


# ------------------------------------------------------------------------------------------------------------ autograd behaviour

def test_gradients_bitwise_repeatable_and_accumulate(dev):
    mc, _ = _tiny(dev)
    kernel = mc.kernel
    torch.manual_seed(8)
    x = torch.randn(70, 15, device=dev)
    _, g1, _, _ = _hip_grads(kernel, (15,), x, None, 21, dev)
    g1 = {k: v.clone() for k, v in g1.items()}
    _, g2, _, _ = _hip_grads(kernel, (15,), x, None, 21, dev)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # a second backward without zero_grad: torch accumulates g + g, exactly twice the first
    _, g3, _, _ = _hip_grads(kernel, (15,), x, None, 21, dev, zero=False)
    for k in g1:
        assert torch.equal(g3[k], 2 * g1[k]), k
    kernel.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in kernel.parameters())


def test_sgd_trajectory_matches_float64_oracle_and_repacks(dev):
    """Ten SGD steps on the device and on the float64 oracle from the same batches and draws; then the sampling forward (sda_mlp_fwd) with
    the updated weights equals the oracle's: the plan re-packed its slabs after each step."""
    mc, cfg = _tiny(dev)
    kernel = mc.kernel
    names = [k for k, _ in kernel.named_parameters()]
    sd64 = {k: v.detach().double().cpu().clone() for k, v in kernel.state_dict().items()}
    sde = VPSDE(kernel, shape=(15,)).to(dev)
    opt = torch.optim.SGD(kernel.parameters(), lr=0.05)
    sched = O.Schedule()
    gen = torch.Generator().manual_seed(9)
    for step in range(10):
        x = torch.randn(4, 15, generator=gen).to(dev)
        torch.manual_seed(100 + step)
        with training.parameter_gradients(mlp=True):
            sde.loss(x).backward()
        opt.step()
        opt.zero_grad()
        torch.manual_seed(100 + step)
        t = torch.rand(4, device=dev).double().cpu()
        e = torch.randn(4, 15, device=dev).double().cpu()
        leaves = {k: sd64[k].clone().requires_grad_(k in names) for k in sd64}
        xt = sched.mu(t.reshape(-1, 1)) * x.double().cpu() + sched.sigma(t.reshape(-1, 1)) * e
        loss = (O.score_net(leaves, '', cfg, xt, t) - e).square().mean()
        grads = torch.autograd.grad(loss, [leaves[k] for k in names])
        for k, gr in zip(names, grads):
            sd64[k] = sd64[k] - 0.05 * gr
    params = dict(kernel.named_parameters())
    for k in names:
        ref = sd64[k]
        assert (params[k].detach().double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), k
    xq = torch.randn(3, 15, generator=gen)
    tq = torch.rand(3, generator=gen)
    with torch.no_grad():
        got = kernel(xq.to(dev), tq.to(dev)).cpu()
    assert rel_err(got, O.score_net(sd64, '', cfg, xq.double(), tq.double())) <= 1e-4


def test_utils_loop_trains_a_scorenet(dev):
    from sda_amd.utils import loop
    mc, _ = _tiny(dev)
    kernel = mc.kernel
    before = {k: p.detach().clone() for k, p in kernel.named_parameters()}
    sde = VPSDE(kernel, shape=(15,)).to(dev)
    gen = torch.Generator().manual_seed(10)
    data = [(torch.randn(15, generator=gen), {}) for _ in range(128)]
    out = list(loop(sde, data, data[:32], epochs=2, batch_size=64, learning_rate=1e-3, device=dev))
    assert len(out) == 2
    for lt, lv, _lr in out:
        assert torch.isfinite(torch.tensor([lt, lv])).all()
    assert all(not torch.equal(before[k], p.detach()) for k, p in kernel.named_parameters())
    assert not training.enabled() and not training.mlp_enabled()


def test_sampling_bitwise_unchanged_by_the_mlp_switch(dev):
    """One guided evaluation of the local net (GaussianScore over MCScoreNet) with enable(mlp=True) on == the same evaluation with the
    switch off, bitwise: the guidance VJP runs under input_only()."""
    from sda_amd.score import GaussianScore
    mc, _ = _tiny(dev)
    sde = VPSDE(mc, shape=(9, 3)).to(dev)
    torch.manual_seed(13)
    x = torch.randn(4, 9, 3, device=dev)
    y = torch.randn(4, 3, 3, device=dev)
    t = torch.tensor(0.4, device=dev)
    guided = GaussianScore(y, A=lambda v: v[..., ::4, :], std=0.1, sde=sde)

    def run():
        out = guided(x.clone(), t)
        torch.cuda.synchronize()
        return out.detach().clone()
    off = run()
    training.enable(mlp=True)
    try:
        on = run()
    finally:
        training.disable()
    assert torch.equal(on, off)
    assert all(p.grad is None for p in mc.parameters())
