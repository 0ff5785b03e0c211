r"""Lorenz experiment helpers (experiments/lorenz/utils.py:22-147 of the reference): the score-network factories, and the
ground truth the evaluation is measured against -- ``make_chain``, ``log_prior``, ``log_likelihood``, the particle-filter
``posterior`` and ``weak_4d_var``."""

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


def make_chain() -> chains.MarkovChain:
    return chains.NoisyLorenz63(dt=0.025)


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


def log_prior(x: Tensor) -> Tensor:
    r"""sum_i log p(x_{i+1} | x_i) of (..., L, 3) trajectories under ``make_chain()`` (experiments/lorenz/utils.py:82-88): one
    ``sda_chain_log_prob`` launch, summed in float64.  An input that requires grad takes the torch-ops rk4, which autograd
    differentiates (``weak_4d_var``)."""
    chain = make_chain()
    if torch.is_grad_enabled() and x.requires_grad:
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


def weak_4d_var(x: Tensor, y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1,
                iterations: int = 16) -> Tensor:
    r"""Weak-constraint 4D-Var by L-BFGS on the log-posterior (experiments/lorenz/utils.py:126-147); torch autograd around
    ``log_prior``'s differentiable route."""
    x_b = x[0]
    x = torch.nn.Parameter(x.clone())
    optimizer = torch.optim.LBFGS((x,))

    def closure():
        optimizer.zero_grad()
        loss = (x[0] - x_b).square().sum() - log_prior(x) - log_likelihood(y, x, A, sigma, step)
        loss.backward()
        return loss

    for _ in range(iterations):
        optimizer.step(closure)

    return x.data
