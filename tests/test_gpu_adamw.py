"""GPU: the fused AdamW step that keeps the ResMLP weight slabs packed (csrc/optim.hip; sda_amd.training.AdamW).

Kernel level: the pack epilogue against the host packer, the arithmetic against float64 (yardstick: torch.optim.AdamW on the device)
and against the host emulator, bitwise.  Optimizer level: descriptor splitting, untouched parameters, the plan / version protocol on
ScoreNet, a wide ResMLP, MCScoreNet with a guided evaluation, ``utils.loop(fused=True)`` and a U-Net (the convolution caches)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from sda_amd import _lib, mlp, ops, training
from sda_amd.nn import ResMLP
from sda_amd.score import GaussianScore, MCScoreNet, ScoreNet, ScoreUNet, VPSDE
from tests import adamw_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _step(d):
    assert _lib.load().sda_adamw_step(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ kernel level

@pytest.mark.parametrize('in_f,out_f', A.PACK_SHAPES, ids=lambda v: str(v))
def test_pack_matches_the_host_packer(dev, in_f, out_f):
    """One step with lr = 1e-2 from zeroed slabs: the destinations are, bitwise and padding included, mlp._slab of the updated weight read
    back (forward and transposed) and the updated bias in its padded row."""
    c = A.pack_case(in_f, out_f, dev)
    W0 = c['W'].clone()
    _step(A.pack_desc(c, 1e-2, A.WD))
    assert not torch.equal(c['W'], W0)
    A.check_pack(c)


def _device_five_steps(params, grads, dev):
    ps = [p.clone().to(dev) for p in params]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for t, lr in enumerate(A.LRS, start=1):
        gs = [g.to(dev) for g in grads[t - 1]]
        _step(A.desc(list(zip(ps, gs, ms, vs)), lr, A.WD, t))
    return [(p.cpu(), m.cpu(), v.cpu()) for p, m, v in zip(ps, ms, vs)]


@pytest.fixture(scope='module')
def five_steps(dev):
    """Per gradient scale: (inputs, the device result), computed once."""
    out = {}
    for scale in A.SCALES:
        params, grads = A.arithmetic_inputs(scale)
        out[scale] = (params, grads, _device_five_steps(params, grads, dev))
    return out


@pytest.mark.parametrize('scale', A.SCALES)
def test_arithmetic_against_float64(dev, five_steps, scale):
    """The five-step case of tests/test_adamw_host.py on the device, same rule; the yardstick is torch.optim.AdamW(foreach=False) on the
    device."""
    params, grads, got = five_steps[scale]
    worst = A.check_against_float64(got, A.torch_adamw(params, grads, dev), A.replay64(params, grads))
    print(f'scale {scale}: worst p error {worst[0]:.3e} (torch {worst[1]:.3e})')


@pytest.mark.parametrize('scale', A.SCALES)
def test_device_equals_the_emulator_bitwise(five_steps, scale):
    params, grads, got = five_steps[scale]
    for n, (g3, e3) in enumerate(zip(got, A.emulate_five_steps(A.load_emu(), params, grads))):
        for name, g, e in zip('pmv', g3, e3):
            assert torch.equal(g, e), (n, name, float((g - e).abs().max()))


# ------------------------------------------------------------------------------------------------------------ optimizer level

def _first_step(p, g, lr, wd):
    """The first AdamW step in float64: after the bias corrections m = g and sqrt(v) = |g|."""
    p, g = p.double(), g.double()
    return p * (1 - lr * wd) - lr * g / (g.abs() + A.EPS)


def test_33_tensors_take_two_launches_and_grad_none_is_untouched(dev, monkeypatch):
    torch.manual_seed(0)
    ps = [nn.Parameter(torch.randn(n + 1, device=dev)) for n in range(33)] + [nn.Parameter(torch.randn(7, device=dev))]
    before = [p.detach().clone() for p in ps]
    versions = [p._version for p in ps]
    for p in ps[:33]:
        p.grad = torch.randn_like(p)
    launches = []
    real = ops.adamw_step
    monkeypatch.setattr(ops, 'adamw_step', lambda d: (launches.append(d.ntensor), real(d))[1])
    opt = training.AdamW(ps, lr=1e-2, weight_decay=A.WD)
    opt.step()
    torch.cuda.synchronize()
    assert launches == [32, 1]
    for n, (p, b) in enumerate(zip(ps[:33], before)):
        assert (p.detach().double() - _first_step(b, p.grad, 1e-2, A.WD)).abs().max().item() <= 1e-6, n
        assert p._version == versions[n] + 1 and float(opt.state[p]['step']) == 1.0
    assert torch.equal(ps[33].detach(), before[33]) and ps[33]._version == versions[33]
    assert ps[33] not in opt.state
    # a non-contiguous gradient is made contiguous; a non-contiguous parameter is refused
    q = nn.Parameter(torch.randn(6, 4, device=dev))
    q.grad = torch.randn(4, 6, device=dev).t()
    q0 = q.detach().clone()
    training.AdamW([q], lr=1e-2, weight_decay=0.0).step()
    assert (q.detach().double() - _first_step(q0, q.grad, 1e-2, 0.0)).abs().max().item() <= 1e-6
    r = nn.Parameter(torch.randn(4, 6, device=dev).t())
    r.grad = torch.randn_like(r)
    with pytest.raises(ValueError, match='contiguous'):
        training.AdamW([r]).step()


def _count_slab_calls(monkeypatch):
    calls = []
    real = mlp._slab
    monkeypatch.setattr(mlp, '_slab', lambda W: (calls.append(1), real(W))[1])
    return calls


def _check_plans(net):
    """Every ResMLP's plan holds, bitwise, what a freshly constructed plan packs from the current parameters."""
    n = 0
    for m in net.modules():
        if isinstance(m, ResMLP):
            plan = mlp._fused_plan(list(m))
            fresh = mlp._FusedPlan(list(m))
            fresh._pack()
            assert plan._key == fresh._key
            assert plan.w_off == fresh.w_off and plan.b_off == fresh.b_off
            assert torch.equal(plan.wf, fresh.wf) and torch.equal(plan.wb, fresh.wb) and torch.equal(plan.bias, fresh.bias)
            n += 1
    assert n


def _train_three_steps(net, loss_fn, monkeypatch, **kw):
    """Three steps with training.AdamW(net=net): the plans stay packed without the host packer, versions rise."""
    opt = training.AdamW(net.parameters(), lr=1e-2, weight_decay=A.WD, net=net, **kw)
    calls = _count_slab_calls(monkeypatch)
    for step in range(3):
        versions = {k: p._version for k, p in net.named_parameters()}
        before = len(calls)
        torch.manual_seed(20 + step)
        with training.parameter_gradients(mlp=True):
            loss_fn().backward()
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        if step:
            assert len(calls) == before, f'step {step + 1}: the host packer ran'
        after = len(calls)
        _check_plans(net)                                    # (the fresh plan packs on the host: not counted against the step)
        del calls[after:]
        for k, p in net.named_parameters():
            assert p._version > versions[k], k
    return opt


def _nets():
    return {'scorenet': lambda: (ScoreNet(5, embedding=8, hidden_features=(16,)), 5),
            'wide': lambda: (ResMLP(47, 15, hidden_features=(256,), activation=nn.SiLU), 47)}


@pytest.mark.parametrize('name', ['scorenet', 'wide'])
def test_three_steps_keep_the_plan_packed(dev, monkeypatch, name):
    torch.manual_seed(1)
    net, width = _nets()[name]()
    net = net.to(dev)
    x = torch.randn(4, width, device=dev)
    if name == 'scorenet':
        sde = VPSDE(net, shape=(width,)).to(dev)
        loss_fn = lambda: sde.loss(x)
        evaluate = lambda n: n(x, torch.full((4,), 0.3, device=dev))
    else:
        assert [(k, i, o) for k, i, o, _ in mlp._fused_plan(list(net)).gemms] == [(0, 47, 256), (1, 256, 256), (2, 256, 256), (0, 256, 15),
                                                                                (1, 15, 15), (2, 15, 15)]
        loss_fn = lambda: net(x).square().mean()
        evaluate = lambda n: n(x)
    start = {k: p.detach().clone() for k, p in net.named_parameters()}
    _train_three_steps(net, loss_fn, monkeypatch)
    assert all(not torch.equal(start[k], p.detach()) for k, p in net.named_parameters())
    calls = _count_slab_calls(monkeypatch)
    with torch.no_grad():
        got = evaluate(net)
        assert not calls                                     # (the next forward did not repack either)
        ref = evaluate(copy.deepcopy(net))
        assert calls                                         # (the copy has its own plan, packed on the host)
    assert torch.equal(got, ref)


def test_mcscorenet_steps_then_guided_evaluation(dev, monkeypatch):
    """The fused window path of the samplers sees the weights the optimizer wrote."""
    torch.manual_seed(2)
    mc = MCScoreNet(features=3, order=2, embedding=8, hidden_features=[16] * 2, activation=nn.SiLU).to(dev)
    sde = VPSDE(mc, shape=(9, 3)).to(dev)
    x1 = torch.randn(1, 9, 3, device=dev)
    x = torch.randn(4, 9, 3, device=dev)
    y = torch.randn(4, 3, 3, device=dev)
    t = torch.tensor(0.4, device=dev)

    def guided(net):
        out = GaussianScore(y, A=lambda v: v[..., ::4, :], std=0.1, sde=VPSDE(net, shape=(9, 3)).to(dev))(x.clone(), t)
        torch.cuda.synchronize()
        return out.detach().clone()
    first = guided(mc)                                       # (the window path has run, and cached, before the training)
    _train_three_steps(mc, lambda: sde.loss(x1), monkeypatch)
    got = guided(mc)
    assert not torch.equal(got, first)
    assert torch.equal(got, guided(copy.deepcopy(mc)))


def test_loop_fused_trains_and_the_default_stays_torch(dev, monkeypatch):
    from sda_amd import utils
    built = []
    real_torch, real_ours = torch.optim.AdamW, training.AdamW

    class TorchSpy(real_torch):
        def __init__(self, *a, **kw):
            built.append('torch')
            super().__init__(*a, **kw)

    class OursSpy(real_ours):
        def __init__(self, *a, **kw):
            built.append(('ours', kw.get('net')))
            super().__init__(*a, **kw)
    monkeypatch.setattr(torch.optim, 'AdamW', TorchSpy)
    monkeypatch.setattr(training, 'AdamW', OursSpy)
    gen = torch.Generator().manual_seed(10)
    data = [(torch.randn(5, generator=gen), {}) for _ in range(64)]
    for fused in (True, False):
        torch.manual_seed(3)
        net = ScoreNet(5, embedding=8, hidden_features=(16,)).to(dev)
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        sde = VPSDE(net, shape=(5,)).to(dev)
        kw = {'fused': True} if fused else {}
        del built[:]
        out = list(utils.loop(sde, data, data[:16], epochs=2, batch_size=32, learning_rate=1e-3, device=dev, **kw))
        assert built == ([('ours', sde)] if fused else ['torch'])
        assert len(out) == 2
        for lt, lv, _lr in out:
            assert torch.isfinite(torch.tensor([lt, lv])).all()
        assert all(not torch.equal(before[k], p.detach()) for k, p in net.named_parameters())
        assert not training.enabled() and not training.mlp_enabled()


def test_unet_steps_invalidate_the_conv_caches(dev):
    """Without ``net`` the step is the plain update; the version bump alone makes the convolution weight caches repack."""
    torch.manual_seed(4)
    net = ScoreUNet(3, embedding=8, hidden_channels=(8,), hidden_blocks=(1,), activation=nn.SiLU, spatial=1).to(dev)
    sde = VPSDE(net, shape=(3, 16)).to(dev)
    x = torch.randn(2, 3, 16, device=dev)
    t = torch.full((2,), 0.3, device=dev)
    with torch.no_grad():
        first = net(x, t).clone()                            # (the caches are warm before the training)
    opt = training.AdamW(net.parameters(), lr=1e-2, weight_decay=A.WD)
    for step in range(2):
        torch.manual_seed(30 + step)
        with training.parameter_gradients():
            sde.loss(x).backward()
        assert all(p.grad is not None for p in net.parameters())
        opt.step()
        opt.zero_grad()
    with torch.no_grad():
        got = net(x, t)
        ref = copy.deepcopy(net)(x, t)
    assert not torch.equal(got, first)
    assert torch.equal(got, ref)
