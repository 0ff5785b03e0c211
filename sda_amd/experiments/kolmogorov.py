r"""Kolmogorov chain and score-network factories (experiments/kolmogorov/utils.py:25-81 of the reference)."""

from pathlib import Path
from typing import Callable, Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from ..chains import KolmogorovFlow, MarkovChain
from ..score import MCScoreNet, ScoreUNet
from ..utils import ACTIVATIONS, load_config


def make_chain(grad: str = 'torch') -> MarkovChain:
    r"""The flow the reference's data comes from (kolmogorov/utils.py:25-26): 256 x 256, dt = 0.2 (82 sub-steps).  ``grad='device'``
    differentiates through the kernels (``KolmogorovFlow``)."""
    return KolmogorovFlow(size=256, dt=0.2, grad=grad)


def strong_4d_var(x_b: Tensor, y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1,
                  iterations: int = 16, chain: Optional[MarkovChain] = None) -> Tensor:
    r"""Strong-constraint 4D-Var by L-BFGS over the initial state of a deterministic chain, the counterpart of
    ``experiments.lorenz.weak_4d_var``: minimises :math:`|x_0 - x_b|^2 + \sum |y - A(x_{1:L:step})|^2 / \sigma^2` where
    ``x_{1:L} = chain.trajectory(x0, L)`` and ``L = len(y) * step``.  ``A`` is any differentiable callable on the kept frames
    (``len(y)``, ..., 2, size, size).  ``chain`` defaults to ``make_chain(grad='device')``."""
    chain = make_chain(grad='device') if chain is None else chain
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


def enks(y: Tensor, A: Callable[[Tensor], Tensor] = lambda x: x, sigma: float = 1.0, step: int = 1, members: int = 64, *,
         chain: Optional[MarkovChain] = None, lag: Optional[int] = None, inflation: float = 1.0, burn: int = 0,
         seed: Optional[int] = None, device=None, radius: Optional[float] = None, block=(4, 4), positions=None) -> Tensor:
    r"""Ensemble-Kalman-smoother samples of p(x_{0:L} | y) with ``experiments.lorenz.enks``'s time convention: prior, ``burn``
    transitions, then per observation ``step`` transitions and one stochastic analysis over the window, solved in ensemble space
    (``chains.enks_wide``, at most 128 members); returns ``enks_wide(...)[:, step:]`` on the device, (members, (N - 1) step + 1, 2,
    size, size).  ``A`` is any callable on the members (``Coarsen``, ``Subsample``, ``Vorticity`` and their compositions).  ``chain``
    defaults to ``make_chain()``.

    ``radius=None`` is the global analysis: so few members on so many components are rank-limited.  A number localises it by
    domain (``chains.enks_local``): blocks of ``block`` grid points, each analysed with the observed values within ``2 radius``
    grid points under Gaspari-Cohn weights.  The positions of the observed values come from ``observe.positions(A, event)``
    (``Coarsen``, ``Subsample`` / ``Crop``, ``Vorticity``, ``Pointwise``, ``Mask`` and their compositions); for any other ``A``
    pass ``positions`` (k, 2) yourself."""
    from .. import chains
    chain = make_chain() if chain is None else chain
    if device is None:
        device = y.device if y.is_cuda else torch.device('cuda')
    kw = {'seed': seed} if isinstance(chain, KolmogorovFlow) else {}
    x = chain.prior((members,), device=device, **kw)
    if burn > 0:
        x = chain.trajectory(x, length=burn, last=True)
    if radius is not None:
        if positions is None:
            from .. import observe
            positions = observe.positions(A, tuple(x.shape[1:]))
        return chains.enks_local(chain, x, y.to(device), A, sigma, step, positions=positions, radius=radius, block=block, lag=lag,
                                 inflation=inflation, seed=seed)[:, step:]
    return chains.enks_wide(chain, x, y.to(device), A, sigma, step, lag=lag, inflation=inflation, seed=seed)[:, step:]


class LocalScoreUNet(ScoreUNet):
    r"""Score U-Net with a forcing channel sin(4 * 2 pi (i + 1/2) / size) as its single context channel
    (kolmogorov/utils.py:29-46), defined as the reference defines it: ``forward`` hands ``self.forcing`` on as the context.
    The channel is never concatenated (the head convolution's loader reads it as a broadcast context plane), and inside an
    ``MCScoreNet`` the override is recognised as context-only (``score._context_only_override``), so this class -- and the
    reference's own, when its driver file runs unchanged on this package -- takes the fused window path."""

    def __init__(self, channels: int, size: int = 64, **kwargs):
        super().__init__(channels, 1, **kwargs)
        domain = 2 * torch.pi / size * (torch.arange(size) + 1 / 2)
        self.register_buffer('forcing', torch.sin(4 * domain).expand(1, size, size).clone())

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        return super().forward(x, t, self.forcing)


def make_score(
    window: int = 3,
    embedding: int = 64,
    hidden_channels: Sequence[int] = (64, 128, 256),
    hidden_blocks: Sequence[int] = (3, 3, 3),
    kernel_size: int = 3,
    activation: str = 'SiLU',
    size: int = 64,
    **absorb,
) -> nn.Module:
    score = MCScoreNet(2, order=window // 2)
    score.kernel = LocalScoreUNet(
        channels=window * 2,
        size=size,
        embedding=embedding,
        hidden_channels=hidden_channels,
        hidden_blocks=hidden_blocks,
        kernel_size=kernel_size,
        activation=ACTIVATIONS[activation],
        spatial=2,
        padding_mode='circular',
    )
    return score


def load_score(file: Path, device: str = 'cpu', **kwargs) -> nn.Module:
    state = torch.load(file, map_location=device)
    config = load_config(Path(file).parent)
    config.update(kwargs)
    score = make_score(**config)
    score.load_state_dict(state)
    return score
