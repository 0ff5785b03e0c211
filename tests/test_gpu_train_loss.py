"""Device: the keyed denoising loss (csrc/train_loss.hip; ops.loss_perturb / ops.loss_mse; VPSDE.loss with a training.KeyedLossNoise).

sda_loss_perturb shares its generator with sda_randn_rows and its schedule with sda_vp_schedule and contracts nothing, so t, eps and xt
are compared BITWISE; sda_loss_mse is compared with float64 at the bound its launch geometry gives."""
import pytest
import torch

from sda_amd import ops, score, training
from tests import loss_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9abc
ETA = 1e-3
# (alpha_kind, sigma_kind): lin / cos / exp under VPSDE's sigma, SubVPSDE's and SubSubVPSDE's under cos
KINDS = [(0, 0), (1, 0), (2, 0), (1, 1), (1, 2)]
# (5, 21): the scalar tail; (3, 640): the 16-byte path; (1, 1): one element; (2, 2052): two chunks of a row, the second one short
SHAPES = [(5, 21), (3, 640), (1, 1), (2, 2052)]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('row0,step,on_device', [(0, 0, False), (7, 3, False), (0, 0, True), (7, 3, True)])
def test_perturb_is_bitwise_the_keyed_draws_and_the_shared_schedule(dev, shape, row0, step, on_device):
    rows, per_row = shape
    x = torch.randn(shape, device=dev)
    counter = torch.full((1,), step, device=dev, dtype=torch.int64) if on_device else None
    for ak, sk in KINDS:
        k = R.k_of(ak, ETA)
        # (a by-value step that must be ignored when the device counter is given)
        t, eps, xt = ops.loss_perturb(x, SEED, row0, ak, ETA, k, sk, step=99 if on_device else step, step_dev=counter)
        assert t.shape == (rows,) and eps.shape == x.shape and xt.shape == x.shape
        assert torch.equal(t.cpu(), torch.from_numpy(R.t_rows(rows, SEED, row0, step)))
        assert torch.equal(eps, ops.randn_rows(torch.empty_like(x), SEED, row0, draw=2 * step))
        ms = torch.stack([ops.vp_schedule(t[b:b + 1], ak, ETA, k, sk) for b in range(rows)])
        assert torch.equal(xt, ms[:, 0:1] * x + ms[:, 1:2] * eps), (ak, sk)
    assert float(t.min()) > 0.0 and float(t.max()) < 1.0
    if counter is not None:
        assert int(counter) == step                             # (the launch reads the counter, it never advances it)


def test_perturb_rows_are_keyed_on_the_global_row(dev):
    """Rows 7 .. 9 of a draw from row0 = 0 are rows 0 .. 2 of the draw from row0 = 7; another step gives other draws."""
    x = torch.randn(10, 12, device=dev)
    k = R.k_of(1, ETA)
    t0, e0, _ = ops.loss_perturb(x, SEED, 0, 1, ETA, k, 0, step=2)
    t7, e7, _ = ops.loss_perturb(x[7:], SEED, 7, 1, ETA, k, 0, step=2)
    assert torch.equal(t0[7:], t7) and torch.equal(e0[7:], e7)
    t1, e1, _ = ops.loss_perturb(x, SEED, 0, 1, ETA, k, 0, step=3)
    assert not torch.equal(t0, t1) and not torch.equal(e0, e1)
    assert len(set(t0.tolist())) == 10


@pytest.mark.parametrize('numel', [1, 105, 7680, 2 ** 20 + 3])
def test_mse_is_reproducible_and_within_the_geometry_bound(dev, numel):
    """Loss: every term passes through at most L additions (sda_loss_mse_plan) after the rounding of its difference and of its square, and
    the mean is one more rounding; all terms are non-negative, so the relative error is at most (L + 3) 2^-24.  Cotangent: the
    difference, the fp32 scale 2 / numel and their product round once each: 3 * 2^-24 |g|."""
    gen = torch.Generator(device=dev).manual_seed(numel)
    out, eps = torch.randn(numel, device=dev, generator=gen), torch.randn(numel, device=dev, generator=gen)
    blocks, chain = ops.loss_mse_plan(numel)
    assert (blocks, chain) == R.mse_chain(numel)
    loss, g = ops.loss_mse(out, eps)
    loss2, g2 = ops.loss_mse(out, eps)
    assert loss.shape == () and torch.equal(loss, loss2) and torch.equal(g, g2)
    ref, g_ref = R.mse64(out, eps)
    err = abs(float(loss.double()) - ref) / ref
    print(f'numel {numel}: blocks {blocks}, chain {chain}, loss rel. error {err:.3e} (bound {(chain + 3) * 2.0 ** -24:.3e})')
    assert err <= (chain + 3) * 2.0 ** -24
    g_err = (g.double().cpu() - g_ref).abs()
    print(f'numel {numel}: cotangent max error / bound {float((g_err / (3 * 2.0 ** -24 * g_ref.abs()).clamp_min(1e-300)).max()):.3f}')
    assert bool((g_err <= 3 * 2.0 ** -24 * g_ref.abs()).all())
    only, none = ops.loss_mse(out, eps, with_g=False)
    assert none is None and torch.equal(only, loss)


def test_mse_takes_the_scalar_path_on_an_unaligned_tensor(dev):
    """numel % 4 == 0 but the storage starts 4 bytes off a 16-byte boundary: the scalar path, two full chunks and a short one; same bounds."""
    base_o, base_e = torch.randn(8201, device=dev), torch.randn(8201, device=dev)
    o, e = base_o[1:], base_e[1:]
    assert o.data_ptr() % 16 == 4 and o.numel() % 4 == 0
    loss, g = ops.loss_mse(o, e)
    ref, g_ref = R.mse64(o, e)
    _blocks, chain = ops.loss_mse_plan(o.numel())
    assert abs(float(loss.double()) - ref) / ref <= (chain + 3) * 2.0 ** -24
    assert bool(((g.double().cpu() - g_ref).abs() <= 3 * 2.0 ** -24 * g_ref.abs()).all())


def test_autograd_function_returns_the_cotangent(dev):
    out = torch.randn(6, 35, device=dev, requires_grad=True)
    eps = torch.randn(6, 35, device=dev)
    _loss, g = ops.loss_mse(out.detach(), eps)
    loss = score._KeyedMSE.apply(out, eps)
    loss.backward()
    assert torch.equal(out.grad, g)
    out.grad = None
    (0.5 * score._KeyedMSE.apply(out, eps)).backward()
    half = 0.5 * g.double()
    assert bool(((out.grad.double() - half).abs() <= 2.0 ** -23 * half.abs()).all())          # 1 ulp


def test_vpsde_loss_takes_the_keyed_route_only_when_asked(dev):
    """With loss_noise set the loss is a function of (seed, step) -- not of torch's generator, which it leaves alone --, equals the
    float64 loss of the rebuilt draws, and keeps the reference's weighted expression; without it the route is torch's."""
    torch.manual_seed(0)
    net = score.ScoreNet(5, embedding=8, hidden_features=(16,)).to(dev)
    sde = score.VPSDE(net, shape=(5,)).to(dev)
    x = torch.randn(7, 5, device=dev)
    assert score.VPSDE.loss_noise is None and sde.loss_noise is None
    noise = training.KeyedLossNoise(11, row0=3)
    sde.loss_noise = noise
    noise.step = 2
    state = torch.cuda.get_rng_state(dev)
    with torch.no_grad():
        a = sde.loss(x)
        torch.manual_seed(123)
        b = sde.loss(x)
        assert torch.equal(a, b) and noise.step == 2
        k = R.k_of(1, sde.eta)
        t, eps, xt = ops.loss_perturb(x, 11, 3, 1, sde.eta, k, 0, step=2)
        ref, _ = R.mse64(net(xt, t), eps)
        assert abs(float(a) - ref) <= 64 * 2.0 ** -24 * ref
        w = torch.rand(7, 5, device=dev)
        err = (net(xt, t) - eps).square()
        assert torch.equal(sde.loss(x, w=w), (err * w).mean() / w.mean())
        noise.step = 3
        assert not torch.equal(sde.loss(x), a)
    torch.cuda.set_rng_state(state, dev)
    sde.loss_noise = None
    with torch.no_grad():
        torch.manual_seed(5)
        c = sde.loss(x)
        torch.manual_seed(5)
        assert torch.equal(sde.loss(x), c)
        torch.manual_seed(6)
        assert not torch.equal(sde.loss(x), c)
