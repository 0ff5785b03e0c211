"""Device: a replayed training step that draws its own batches (training.GraphedStep(data=ds, batch_size=B); utils.loop over a
sda_amd.data.DeviceTrajectories).

The yardstick is the route tests/test_gpu_graphed_step.py pins -- a GraphedStep WITHOUT ``data=`` -- fed by hand with the batches a twin
dataset draws: the self-feeding stepper must be bitwise that route (parameters, both AdamW moments, ``loss_sum``, ``state_dict()``).  The
two tiny nets of that file are restated here."""
import copy

import pytest
import torch

from sda_amd import data, training, utils
from sda_amd.experiments.lorenz import make_global_score, make_local_score
from sda_amd.score import VPSDE

pytestmark = pytest.mark.gpu

SEED, DATA_SEED, LR, WD = 17, 17, 1e-3, 1e-2          # (the dataset reuses the loss seed: the counter layouts keep the draws apart)
N, LENGTH, BATCH = 10, 12, 4


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _local():
    """The Lorenz local ScoreNet on flattened windows of 3 frames x 3 values."""
    return make_local_score(window=3, embedding=8, width=32, depth=2), dict(window=3, flatten=True), (9,), dict(mlp=True)


def _global():
    """The single-level 1-D U-Net on windows of 9 frames."""
    return make_global_score(embedding=8, hidden_channels=(8,), hidden_blocks=(1,)), dict(window=9), (9, 3), dict(mlp=True, net1d=True)


NETS = {'local': _local, 'global': _global}


class Case:
    def __init__(self, name, dev):
        torch.manual_seed(sum(map(ord, name)))
        self.name, self.dev = name, dev
        net, self.ds_kw, self.shape, self.route = NETS[name]()
        self.start = copy.deepcopy(net.state_dict())
        self.x = torch.randn(N, LENGTH, 3)

    def dataset(self, n=N):
        return data.DeviceTrajectories(self.x[:n], seed=DATA_SEED, device=self.dev, **self.ds_kw)

    def fresh(self):
        net = NETS[self.name]()[0]
        net.load_state_dict(self.start)
        net = net.to(self.dev)
        sde = VPSDE(net.kernel if self.name == 'local' else net, shape=self.shape).to(self.dev)
        return sde, training.AdamW(sde.parameters(), lr=LR, weight_decay=WD, net=sde)


def _snapshot(sde, opt, stepper):
    sd = opt.state_dict()
    out = {f'p.{k}': v.detach().clone() for k, v in sde.eps.state_dict().items()}
    for i, st in sd['state'].items():
        out.update({f's.{i}.{k}': v.detach().clone().to(stepper.loss_sum.device) for k, v in st.items()})
    out['loss_sum'] = stepper.loss_sum.clone()
    return out, [{k: v for k, v in g.items() if k != 'params'} for g in sd['param_groups']]


def _assert_same(a, b):
    (ta, ga), (tb, gb) = a, b
    assert ga == gb
    assert ta.keys() == tb.keys()
    bad = [k for k in ta if not torch.equal(ta[k], tb[k])]
    assert not bad, bad


@pytest.fixture(scope='module', params=sorted(NETS))
def case(request, dev):
    return Case(request.param, dev)


def test_self_feeding_stepper_equals_the_hand_fed_one(case):
    """Seven steps over N = 10 windows at batch 4 -- two epochs (4, 4, 2 rows) and one step more: a warm-up, four replays, two short
    batches run uncaptured -- against a GraphedStep without data= handed ``twin.draw(4)``: everything bitwise."""
    sde, opt = case.fresh()
    ds = case.dataset()
    stepper = training.GraphedStep(sde, opt, seed=SEED, data=ds, batch_size=BATCH, **case.route)
    losses = [stepper.step().clone() for _ in range(7)]
    assert stepper._graph is not None and stepper._shape == (BATCH,) + case.shape
    assert ds.cursor.item() == 7 and ds._s == 7 and stepper.noise.step == 7

    ref_sde, ref_opt = case.fresh()
    twin = case.dataset()
    ref = training.GraphedStep(ref_sde, ref_opt, seed=SEED, **case.route)
    shapes, ref_losses = [], []
    for _ in range(7):
        x = twin.draw(BATCH)
        shapes.append(x.shape[0])
        ref_losses.append(ref.step(x).clone())
    assert shapes == [4, 4, 2, 4, 4, 2, 4]
    assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses))
    assert len({float(l) for l in losses}) == 7
    _assert_same(_snapshot(sde, opt, stepper), _snapshot(ref_sde, ref_opt, ref))
    with pytest.raises(TypeError):
        stepper.step(torch.zeros(BATCH, *case.shape, device=case.dev))
    with pytest.raises(TypeError):
        ref.step()


def test_a_dataset_smaller_than_the_batch_trains_uncaptured(case):
    """N = 3 < batch: every batch is the epoch's short one, no graph is ever captured, the steps still match the hand-fed route."""
    sde, opt = case.fresh()
    stepper = training.GraphedStep(sde, opt, seed=SEED, data=case.dataset(3), batch_size=BATCH, **case.route)
    ref_sde, ref_opt = case.fresh()
    twin, ref = case.dataset(3), training.GraphedStep(ref_sde, ref_opt, seed=SEED, **case.route)
    for _ in range(2):
        assert torch.equal(stepper.step(), ref.step(twin.draw(BATCH)))
    assert stepper._graph is None


def _hand_driven_loop(case, epochs):
    """utils.loop(graph=True)'s training half by hand: the hand-fed stepper, LambdaLR('linear') stepped once per epoch."""
    sde, opt = case.fresh()
    twin = case.dataset()
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=utils._SCHEDULES['linear'](epochs))
    stepper = training.GraphedStep(sde, opt, seed=SEED, **case.route)
    opt._opt_called = True
    means = []
    for _ in range(epochs):
        stepper.loss_sum.zero_()
        n = 0
        for x, _kw in twin.batches(BATCH):
            stepper.step(x)
            n += 1
        means.append((stepper.loss_sum / n).item())
        sched.step()
    return sde, means


def test_loop_draws_inside_the_graph_and_equals_the_hand_driven_twin(case):
    sde, _ = case.fresh()
    train, valid = case.dataset(), data.DeviceTrajectories(case.x[:5], seed=DATA_SEED + 1, device=case.dev, **case.ds_kw)
    got = list(utils.loop(sde, train, valid, epochs=2, batch_size=BATCH, learning_rate=LR, weight_decay=WD, device=case.dev, graph=True,
                          seed=SEED, net1d=case.route.get('net1d', False)))
    assert not training.enabled()
    assert len(got) == 2 and all(torch.isfinite(torch.tensor(t)).all() for t in got)
    assert [t[2] for t in got] == [LR, LR / 2]
    assert train.cursor.item() == 6 and valid.cursor.item() == 4          # (3 + 3 training batches, 2 + 2 validation batches)
    want_sde, means = _hand_driven_loop(case, 2)
    assert [t[0] for t in got] == means
    for (k, a), (_k, b) in zip(sde.eps.state_dict().items(), want_sde.eps.state_dict().items()):
        assert torch.equal(a, b), k
    untrained, _ = case.fresh()
    assert any(not torch.equal(a, b) for a, b in zip(sde.parameters(), untrained.parameters()))


def test_loop_without_graph_runs_on_device_batches(case):
    sde, _ = case.fresh()
    before = [p.detach().clone() for p in sde.parameters()]
    train, valid = case.dataset(), case.dataset(5)
    torch.manual_seed(0)
    got = list(utils.loop(sde, train, valid, epochs=2, batch_size=BATCH, learning_rate=LR, weight_decay=WD, device=case.dev, fused=True,
                          net1d=case.route.get('net1d', False)))
    assert len(got) == 2 and all(torch.isfinite(torch.tensor(t)).all() for t in got)
    assert train.cursor.item() == 6 and valid.cursor.item() == 4
    assert any(not torch.equal(a, b) for a, b in zip(before, sde.parameters()))


def test_refusals(case):
    sde, opt = case.fresh()
    with pytest.raises(ValueError, match='batch_size'):
        training.GraphedStep(sde, opt, seed=0, data=case.dataset())
    with pytest.raises(ValueError, match='batch_size'):
        training.GraphedStep(sde, opt, seed=0, batch_size=4)
    host = data.DeviceTrajectories(case.x, device='cpu', **case.ds_kw)
    with pytest.raises(ValueError, match='lives on'):
        training.GraphedStep(sde, opt, seed=0, data=host, batch_size=4)
