"""Device: a training step replayed as one hipGraph (sda_amd.training.GraphedStep, utils.loop(graph=True)).

The yardstick is the UNCAPTURED keyed route -- ``sde.loss`` with a ``training.KeyedLossNoise``, ``backward()``, ``training.AdamW.step()`` --
which a control first shows to be bitwise repeatable on these nets; a replay must then be bitwise that route: parameters, both moments,
losses, ``state_dict()``.  Three tiny nets: the Lorenz local ScoreNet (mlp=True), the single-level 1-D U-Net (net1d=True, and on the per-layer route) and two
2-D ScoreUNets on the per-layer route."""
import copy

import pytest
import torch
import torch.nn as nn

from sda_amd import ops, training, utils
from sda_amd.experiments.lorenz import make_global_score, make_local_score
from sda_amd.score import GaussianScore, ScoreUNet, VPSDE

pytestmark = pytest.mark.gpu

SEED, LR, WD = 17, 1e-3, 1e-2


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _local():
    """MCScoreNet(3, order=1); as the reference's train_local, the step trains its kernel (a ScoreNet) on flattened windows of 9 values."""
    return make_local_score(window=3, embedding=8, width=32, depth=2), (9,), 6, dict(mlp=True)


def _global():
    return make_global_score(embedding=8, hidden_channels=(8,), hidden_blocks=(1,)), (9, 3), 5, dict(mlp=True, net1d=True)


def _unet2d():
    return ScoreUNet(4, embedding=8, hidden_channels=(32,), hidden_blocks=(1,), activation=nn.SiLU, spatial=2), (4, 8, 8), 3, dict(mlp=True)


def _unet1d():
    """The same 1-D net on the per-layer route."""
    return _global()[:3] + (dict(mlp=True),)


def _unet2d_two_levels():
    """Two levels: a stride-2 head (its parity packings are re-packed inside the graph) and an up-sampling tail."""
    return ScoreUNet(4, embedding=8, hidden_channels=(8, 16), hidden_blocks=(1, 1), activation=nn.SiLU, spatial=2), (4, 8, 8), 3, dict(mlp=True)


NETS = {'local': _local, 'global': _global, 'unet1d': _unet1d, 'unet2d': _unet2d, 'unet2d_two_levels': _unet2d_two_levels}


class Case:
    """One net family: the start state, six batches (the last one a row short) and the learning rate of each step (halved after step 3)."""

    def __init__(self, name, dev):
        torch.manual_seed(sum(map(ord, name)))
        self.make, self.dev = NETS[name], dev
        net, self.shape, self.batch, self.route = self.make()
        self.start = copy.deepcopy(net.state_dict())
        self.xs = [torch.randn(self.batch, *self.shape, device=dev) for _ in range(5)] + [torch.randn(self.batch - 1, *self.shape, device=dev)]
        self.lrs = [LR] * 3 + [LR / 2] * 3

    def fresh(self, state=None):
        net = self.make()[0]
        net.load_state_dict(self.start if state is None else state)
        net = net.to(self.dev)
        sde = VPSDE(getattr(net, 'kernel', net) if self.make is _local else net, shape=self.shape).to(self.dev)
        sde.whole = [net]                                     # (the module the state was loaded into: the MCScoreNet of the local case)
        return sde, training.AdamW(sde.parameters(), lr=LR, weight_decay=WD, net=sde)

    def keyed_loss(self, sde, x, step):
        """The uncaptured keyed loss of training step ``step`` on the training route (grad mode on)."""
        sde.loss_noise = training.KeyedLossNoise(SEED)
        sde.loss_noise.step = step
        try:
            with training.parameter_gradients(**self.route):
                return sde.loss(x)
        finally:
            sde.loss_noise = None

    def uncaptured(self, steps=6):
        sde, opt = self.fresh()
        losses = []
        for s in range(steps):
            opt.param_groups[0]['lr'] = self.lrs[s]
            loss = self.keyed_loss(sde, self.xs[s], s)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach().clone())
        return sde, opt, losses

    def graphed(self, steps=6, rows=2):
        sde, opt = self.fresh()
        stepper = training.GraphedStep(sde, opt, seed=SEED, rows=rows, **self.route)
        losses = []
        for s in range(steps):
            opt.param_groups[0]['lr'] = self.lrs[s]
            losses.append(stepper.step(self.xs[s]).clone())
        return sde, opt, losses, stepper


def _snapshot(sde, opt, losses):
    sd = opt.state_dict()
    out = {f'p.{k}': v.detach().clone() for k, v in sde.eps.state_dict().items()}
    for i, st in sd['state'].items():
        out.update({f's.{i}.{k}': v.detach().clone().to(losses[0].device) for k, v in st.items()})
    out.update({f'loss.{i}': l for i, l in enumerate(losses)})
    return out, [{k: v for k, v in g.items() if k != 'params'} for g in sd['param_groups']]


def _assert_same(a, b):
    (ta, ga), (tb, gb) = a, b
    assert ga == gb
    assert ta.keys() == tb.keys()
    bad = [k for k in ta if not torch.equal(ta[k], tb[k])]
    assert not bad, bad


@pytest.fixture(scope='module', params=sorted(NETS))
def case(request, dev):
    c = Case(request.param, dev)
    c.name = request.param
    c.ref = _snapshot(*c.uncaptured())                       # computed once, shared, never modified
    return c


def test_control_the_uncaptured_keyed_route_is_bitwise_repeatable(case):
    """Two uncaptured keyed runs from the same state and seed: parameters, exp_avg, exp_avg_sq, step counts and losses are bitwise equal
    (nothing in the route draws from a generator or accumulates with atomics), so the replay tests below compare bitwise."""
    _assert_same(_snapshot(*case.uncaptured()), case.ref)
    assert len({float(case.ref[0][f'loss.{i}']) for i in range(6)}) == 6


def test_replay_equals_the_uncaptured_route(case):
    """Six steps through GraphedStep -- a warm-up step, four replays with the table (rows = 2) rebuilt twice and the learning rate halved
    after step 3, then a short last batch run uncaptured -- against the six uncaptured keyed steps: everything bitwise, state_dict()
    and its step counts included."""
    sde, opt, losses, stepper = case.graphed()
    assert stepper._graph is not None and stepper._shape == (case.batch,) + case.shape
    assert all(float(opt.state[p]['step']) < 6 for p in sde.parameters())          # (advanced lazily ...)
    _assert_same(_snapshot(sde, opt, losses), case.ref)                             # (... and brought up to date by state_dict())
    assert all(float(opt.state[p]['step']) == 6 for p in sde.parameters())
    total = torch.zeros((), device=case.dev)
    for l in losses:
        total += l
    assert torch.equal(stepper.loss_sum, total) and stepper.noise.step == 6


def test_no_stale_packing_after_replays(case):
    """After graphed steps the sampling route computes with the trained weights: bitwise a freshly constructed net loaded with them."""
    sde, opt, _losses, _stepper = case.graphed(steps=5)
    x, t = case.xs[0], torch.full((case.batch,), 0.37, device=case.dev)
    sde.eval()
    with torch.no_grad():
        got = sde.eps(x, t).clone()
    twin, _ = case.fresh(copy.deepcopy(sde.whole[0].state_dict()))
    twin.eval()
    with torch.no_grad():
        assert torch.equal(got, twin.eps(x, t))
        start, _ = case.fresh()
        assert not torch.equal(got, start.eps(x, t))
    if case.name == 'local':                                  # the fused window kernels: a guided evaluation and one sampler step
        y, xg = torch.randn(4, 3, 3, device=case.dev), torch.randn(4, 9, 3, device=case.dev)

        def guided(s):
            whole = VPSDE(s.whole[0], shape=(9, 3)).to(case.dev)
            g = VPSDE(GaussianScore(y, A=lambda v: v[..., ::4, :], std=0.1, sde=whole), shape=(9, 3)).to(case.dev)
            torch.manual_seed(3)
            sampler = g.sampler((4,), steps=4)
            sampler.step()
            return g.eps(xg, torch.tensor(0.4, device=case.dev)).clone(), sampler.x.clone()
        for a, b in zip(guided(sde), guided(twin)):
            assert torch.equal(a, b)


def test_a_replay_computes_with_the_current_weights(case):
    """Parameters overwritten in place between two replays: the next replayed loss differs from an untouched instance's and is the
    uncaptured keyed loss at the overwritten parameters."""
    runs = []
    for touch in (False, True):
        sde, opt = case.fresh()
        stepper = training.GraphedStep(sde, opt, seed=SEED, **case.route)
        for s in range(2):
            stepper.step(case.xs[s])
        if touch:
            with torch.no_grad():
                for p in sde.parameters():
                    p.mul_(1.01)
            state = copy.deepcopy(sde.whole[0].state_dict())
        runs.append(stepper.step(case.xs[2]).clone())
    assert not torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0], case.ref[0]['loss.2'])
    at, _ = case.fresh(state)
    assert torch.equal(runs[1], case.keyed_loss(at, case.xs[2], 2).detach())


def test_loop_graph_yields_the_uncaptured_keyed_triples(dev):
    """utils.loop(graph=True) over two epochs of three batches (4, 4 and 3 items) == a hand-driven uncaptured keyed loop with the same
    loaders, optimizer and schedule."""
    from torch.utils.data import DataLoader
    c = Case('local', dev)
    gen = torch.Generator().manual_seed(1)
    train = [(torch.randn(*c.shape, generator=gen), {}) for _ in range(11)]          # (windows, as train_local feeds them)
    valid = train[:4]

    torch.manual_seed(9)
    sde, _ = c.fresh()
    got = list(utils.loop(sde, train, valid, epochs=2, batch_size=4, learning_rate=LR, weight_decay=WD, device=dev, graph=True, seed=SEED))
    assert not training.enabled()

    torch.manual_seed(9)
    sde, _ = c.fresh()
    loaders = [DataLoader(ds, batch_size=4, shuffle=True) for ds in (train, valid)]
    opt = training.AdamW(sde.parameters(), lr=LR, weight_decay=WD, net=sde)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=utils._SCHEDULES['linear'](2))
    want, step = [], 0
    for _ in range(2):
        total, n, lv = torch.zeros((), device=dev), 0, []
        sde.train()
        for x, _kw in loaders[0]:
            loss = c.keyed_loss(sde, x.to(dev), step)
            loss.backward()
            opt.step()
            opt.zero_grad()
            total += loss.detach()
            step, n = step + 1, n + 1
        sde.eval()
        with torch.no_grad():
            for x, _kw in loaders[1]:
                lv.append(sde.loss(x.to(dev)))
        want.append(((total / n).item(), torch.stack(lv).mean().item(), opt.param_groups[0]['lr']))
        sched.step()
    assert got == want


def test_refusals(dev):
    c = Case('local', dev)
    sde, opt = c.fresh()
    with pytest.raises(TypeError, match='AdamW'):
        training.GraphedStep(sde, torch.optim.AdamW(sde.parameters()), seed=0)
    with pytest.raises(ValueError):
        training.GraphedStep(sde, opt, seed=0, rows=0)
    prev = ops.set_multiply('f16x2')
    try:
        with pytest.raises(NotImplementedError, match='fp32 multiply'):
            training.GraphedStep(sde, opt, seed=0)
    finally:
        ops.set_multiply(prev)
