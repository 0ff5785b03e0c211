r"""Lorenz experiment helpers (experiments/lorenz/utils.py:22-147 of the reference): the score-network factories, and the
ground truth the evaluation is measured against -- ``make_chain``, ``log_prior``, ``log_likelihood``, the particle-filter
``posterior`` and ``weak_4d_var`` -- and ``strong_4d_var``, its strong-constraint counterpart.  ``grad='device'`` (opt-in) keeps the
gradients of ``log_prior`` / ``weak_4d_var`` on the chain kernels; every default launches what it always launched."""

from pathlib import Path
from typing import Callable, Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Normal

from .. import chains, metrics, ops
from .._lib import SdaHipError
from ..score import MCScoreNet, MCScoreWrapper, ScoreUNet
from ..utils import ACTIVATIONS, load_config

#: which route the last ``posterior`` call took: 'fused' or 'generic' (tests and the bench tool read it)
LAST_POSTERIOR_ROUTE = None


def make_chain(grad: str = 'torch') -> chains.MarkovChain:
    return chains.NoisyLorenz63(dt=0.025, grad=grad)


def make_global_score(
    embedding: int = 32,
    hidden_channels: Sequence[int] = (64,),
    hidden_blocks: Sequence[int] = (3,),
    activation: str = 'SiLU',
    channels: int = 3,
    **absorb,
) -> nn.Module:
    return MCScoreWrapper(ScoreUNet(channels=channels, embedding=embedding, hidden_channels=hidden_channels,
                                    hidden_blocks=hidden_blocks, activation=ACTIVATIONS[activation], spatial=1))


def make_local_score(
    window: int = 5,
    embedding: int = 32,
    width: int = 128,
    depth: int = 5,
    activation: str = 'SiLU',
    features: int = 3,
    **absorb,
) -> nn.Module:
    return MCScoreNet(features=features, order=window // 2, embedding=embedding, hidden_features=[width] * depth,
                      activation=ACTIVATIONS[activation])


def load_score(file: Path, local: bool = False, device: str = 'cpu', **kwargs) -> nn.Module:
    state = torch.load(file, map_location=device)
    config = load_config(Path(file).parent)
    config.update(kwargs)
    score = make_local_score(**config) if local else make_global_score(**config)
    score.load_state_dict(state)
    return score


class _ChainLogProb(torch.autograd.Function):
    """``ops.chain_log_prob_grad``: value and gradient in the forward's one launch.  The kernel takes no upstream cotangent, so
    backward is one torch multiply of the kept gradient by the cotangent of each trajectory's value."""

    @staticmethod
    def forward(ctx, flat, model):
        value, grad = ops.chain_log_prob_grad(model, flat)
        ctx.save_for_backward(grad)
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        grad, = ctx.saved_tensors
        return grad * gout.to(torch.float32)[:, None, None], None


def log_prior(x: Tensor, *, grad: str = 'torch') -> Tensor:
    r"""sum_i log p(x_{i+1} | x_i) of (..., L, 3) trajectories under ``make_chain()`` (experiments/lorenz/utils.py:82-88): one
    ``sda_chain_log_prob`` launch, summed in float64.  An input that requires grad takes the torch-ops rk4, which autograd
    differentiates (``weak_4d_var``) -- or, with ``grad='device'`` and a float32 device input, one ``sda_chain_log_prob_grad`` launch
    that returns the same value with its gradient (first order only).  ``chains.LAST_CHAIN_GRAD_ROUTE`` records which."""
    chain = make_chain(grad)
    if torch.is_grad_enabled() and x.requires_grad:
        if grad == 'device' and x.is_cuda and x.dtype == torch.float32:
            chains.LAST_CHAIN_GRAD_ROUTE = 'device'
            return _ChainLogProb.apply(x.reshape(-1, *x.shape[-2:]), chain.model()).to(x.dtype).reshape(x.shape[:-2])
        return chain.log_prob(x[..., :-1, :], x[..., 1:, :]).sum(dim=-1)
    ops._dev(x)
    flat = x.reshape(-1, *x.shape[-2:])
    return ops.chain_log_prob(chain.model(), flat).to(x.dtype).reshape(x.shape[:-2])


def log_likelihood(y: Tensor, x: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1) -> Tensor:
    x = x[..., ::step, :]
    log_p = Normal(y, sigma).log_prob(A(x))
    return log_p.sum(dim=(-1, -2))


def posterior(y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1, particles: int = 16384, *,
              fused='auto', device=None, seed: Optional[int] = None) -> Tensor:
    r"""Bootstrap-particle-filter samples of p(x_{0:L} | y) (experiments/lorenz/utils.py:106-123): prior, 64 burn-in
    transitions, then per observation ``step`` transitions, weights and resampling; returns ``bpf(...)[:, step:]`` on the device.

    fused='auto': the fused filter (``chains.bpf_fused``) when ``A`` is a ``chains.AffineObservation`` or probes as one
    (``chains.probe_affine`` -- the reference's ``lambda x: chain.preprocess(x)[..., :1]`` does), else ``metrics.bpf`` around the
    native ``chain.transition``.  fused=True raises if the probe fails; fused=False forces the generic route."""
    global LAST_POSTERIOR_ROUTE
    chain = make_chain()
    if device is None:
        device = y.device if y.is_cuda else torch.device('cuda')
    obs = None
    if fused is True or fused == 'auto':
        obs = chains.probe_affine(A, chain, 3)
        if obs is None and fused is True:
            raise SdaHipError('posterior(fused=True): A is not an affine selection of state components (each output an affine '
                              'function of exactly one component); pass fused=False for the generic filter')
    x = chain.prior((particles,), device=device)
    x = chain.trajectory(x, length=64, last=True, seed=seed)
    y = y.to(device)
    if obs is not None:
        LAST_POSTERIOR_ROUTE = 'fused'
        return chains.bpf_fused(chain, x, y, obs, sigma, step, seed=seed)[:, step:]

    def likelihood(yi, xi):
        w = Normal(yi, sigma).log_prob(A(xi)).sum(dim=-1)
        return torch.softmax(w, 0)

    LAST_POSTERIOR_ROUTE = 'generic'
    return metrics.bpf(x, y, chain.transition, likelihood, step)[:, step:]


def enks(y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1, members: int = 1024, *,
         lag: Optional[int] = None, inflation: float = 1.0, chain: Optional[chains.MarkovChain] = None, burn: int = 64,
         seed: Optional[int] = None, device=None, space: str = 'observation', radius: Optional[float] = None, block: int = 4,
         positions=None) -> Tensor:
    r"""Ensemble-Kalman-smoother samples of p(x_{0:L} | y) with ``posterior``'s time convention and return shape: prior, ``burn``
    transitions, then per observation ``step`` transitions and one stochastic analysis over the window (``chains.enks_fused``);
    returns ``enks_fused(...)[:, step:]`` on the device.  ``A`` must be a ``chains.AffineObservation`` or probe as one
    (``chains.probe_affine``), else this raises as ``posterior(fused=True)`` does.  ``chain`` defaults to ``make_chain()``; any
    ``DiscreteODE`` the kernels serve works (``chains.Lorenz96(n)``), where a particle filter has no hope.

    ``space='ensemble'`` solves the same analysis in ensemble space (``chains.enks_wide``): at most 128 members, and ``A`` is any
    callable on the members; it is not probed.  There ``radius`` (in components; None: the global analysis) localises the
    analysis on the ring (``chains.enks_local``): blocks of ``block`` components, each analysed with the observed values within
    ``2 radius`` under Gaspari-Cohn weights.  The positions of the observed values are those of ``observe.positions`` for an
    ``observe`` operator, else the components a probe finds when ``A`` is a plain selection of them; for anything else pass
    ``positions`` (k,)."""
    if space not in ('observation', 'ensemble'):
        raise ValueError(f"enks: space={space!r}, expected 'observation' or 'ensemble'")
    chain = make_chain() if chain is None else chain
    if device is None:
        device = y.device if y.is_cuda else torch.device('cuda')
    x = chain.prior((members,), device=device)
    obs = chains.probe_affine(A, chain, x.shape[-1]) if space == 'observation' else None
    if obs is None and space == 'observation':
        raise SdaHipError('enks: A is not an affine selection of state components (each output an affine function of exactly one '
                          'component)')
    kw = {'seed': seed} if isinstance(chain, (chains.NoisyLorenz63, chains.LinearGaussian)) else {}
    if burn > 0:
        x = chain.trajectory(x, length=burn, last=True, **kw)
    if radius is not None:
        if space != 'ensemble':
            raise ValueError("enks: radius= localises the ensemble-space analysis; pass space='ensemble'")
        if positions is None:
            positions = _ring_positions(A, chain, x.shape[-1])
        return chains.enks_local(chain, x, y.to(device), A, sigma, step, positions=positions, radius=radius, block=block, lag=lag,
                                 inflation=inflation, seed=seed)[:, step:]
    if space == 'ensemble':
        return chains.enks_wide(chain, x, y.to(device), A, sigma, step, lag=lag, inflation=inflation, seed=seed)[:, step:]
    return chains.enks_fused(chain, x, y.to(device), obs, sigma, step, lag=lag, inflation=inflation, seed=seed)[:, step:]


def _ring_positions(A, chain, d: int):
    """Where on the ring the outputs of ``A`` sit: ``observe.positions`` for an ``observe`` operator, else the components of a
    probed selection (``chains.probe_affine``)."""
    from .. import observe
    if isinstance(A, observe.Observation):
        return observe.positions(A, (d,))[:, 1]
    obs = chains.probe_affine(A, chain, d)
    if obs is None:
        raise SdaHipError('enks: A is not a selection of state components, so the positions of its outputs are not known; pass '
                          'positions=')
    return [float(i) for i in obs.index]


def weak_4d_var(x: Tensor, y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1,
                iterations: int = 16, grad: str = 'torch') -> Tensor:
    r"""Weak-constraint 4D-Var by L-BFGS on the log-posterior (experiments/lorenz/utils.py:126-147); torch autograd around
    ``log_prior``'s differentiable route, which ``grad`` selects."""
    x_b = x[0]
    x = torch.nn.Parameter(x.clone())
    optimizer = torch.optim.LBFGS((x,))

    def closure():
        optimizer.zero_grad()
        loss = (x[0] - x_b).square().sum() - log_prior(x, grad=grad) - log_likelihood(y, x, A, sigma, step)
        loss.backward()
        return loss

    for _ in range(iterations):
        optimizer.step(closure)

    return x.data


def strong_4d_var(x_b: Tensor, y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1,
                  iterations: int = 16, chain: Optional[chains.MarkovChain] = None) -> Tensor:
    r"""Strong-constraint 4D-Var by L-BFGS over the initial state of a deterministic chain, with the signature and objective of
    ``experiments.kolmogorov.strong_4d_var``: minimises :math:`|x_0 - x_b|^2 + \sum |y - A(x_{1:L:step})|^2 / \sigma^2` where
    ``x_{1:L} = chain.trajectory(x0, L)`` and ``L = len(y) * step``.  ``chain`` defaults to ``chains.Lorenz63(dt=0.025,
    grad='device')``: per closure one forward launch and one adjoint launch, whatever L.  Any ``DiscreteODE`` serves (``Lorenz96``)."""
    chain = chains.Lorenz63(dt=0.025, grad='device') if chain is None else chain
    length = len(y) * step
    x0 = torch.nn.Parameter(x_b.detach().clone())
    optimizer = torch.optim.LBFGS((x0,))

    def closure():
        optimizer.zero_grad()
        loss = (x0 - x_b).square().sum() + ((y - A(chain.trajectory(x0, length)[::step])).square() / sigma ** 2).sum()
        loss.backward()
        return loss

    for _ in range(iterations):
        optimizer.step(closure)

    return x0.data
