r"""Damped-spring experiment helpers, the counterpart of ``experiments/lorenz.py`` for the one chain of sda/mcs.py that is linear and
Gaussian: everything here is EXACT.  ``posterior`` draws from p(x_{0:L} | y) with a forward filter and a backward sampler
(csrc/lgss.hip) instead of a particle filter, ``log_evidence`` is log p(y) in closed form, and ``ExactScore`` is the analytic
``eps`` of the VP-noised trajectory, a drop-in for a trained score network.

Time convention (experiments/lorenz/utils.py:106-123): the chain starts from its prior and runs ``burn`` transitions; observation
``j`` sees the state ``(j + 1) * step`` transitions later; the returned trajectory starts at the first observed state.  So ``y`` with
N rows gives ``T + 1 = (N - 1) * step + 1`` states, observation ``j`` sits at index ``j * step``, and the first returned state is
Gaussian with the prior's moments pushed through ``burn + step`` transitions (``initial``)."""

import math
from typing import Callable, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Normal

from .. import chains, ops
from .._lib import SdaHipError

_IDENTITY = lambda x: x  # noqa: E731


def make_chain() -> chains.LinearGaussian:
    return chains.DampedSpring(dt=0.01)


def _f64(chain):
    return tuple(v.double() for v in (chain.A, chain.b, chain.Sigma_x, chain.mu_0, chain.Sigma_0))


def initial(burn: int = 64, step: int = 1, chain: Optional[chains.LinearGaussian] = None) -> Tuple[Tensor, Tensor]:
    """Mean and covariance (float64, host) of the first returned state: the prior pushed through ``burn + step`` transitions."""
    A, b, Q, m, P = _f64(make_chain() if chain is None else chain)
    for _ in range(burn + step):
        m = A @ m + b
        P = A @ P @ A.T + Q
        P = 0.5 * (P + P.T)
    return m, P


def _observation(A, chain) -> Tuple[Tensor, Tensor]:
    got = chains.probe_linear(A, chain, chain.d)
    if got is None:
        raise SdaHipError('the exact posterior needs an affine observation A(x) = H x + c with 1 to 8 outputs: this callable is not one')
    return got


def _model64(chain, A, sigma: float, step: int, burn: int):
    H, c = _observation(A, chain)
    Am, b, Q, _, _ = _f64(chain)
    m0, P0 = initial(burn, step, chain)
    return ops.lgss_model64(Am, b, Q, m0, P0, H, c, sigma)


def _filter(y: Tensor, A, sigma: float, step: int, burn: int, chain, device=None):
    chain = make_chain() if chain is None else chain
    if y.dim() not in (2, 3):
        raise SdaHipError(f'observations of shape {tuple(y.shape)}, expected (N, k) or (B, N, k)')
    if device is None:
        device = y.device if y.is_cuda else torch.device('cuda')
    model = _model64(chain, A, sigma, step, burn)
    yb = (y if y.dim() == 3 else y[None]).to(device=device, dtype=torch.float32)
    table = ops.lgss_tables(model, step, yb.shape[1], device=device)
    mean, logz = ops.lgss_filter(model, table, yb, step)
    return model, table, mean, logz


def posterior(y: Tensor, A: Callable[[Tensor], Tensor] = _IDENTITY, sigma: float = 1.0, step: int = 1, samples: int = 1024, *,
              burn: int = 64, seed: Optional[int] = None, chain: Optional[chains.LinearGaussian] = None, device=None) -> Tensor:
    r"""Exact samples of p(x_{0:L} | y): y (N, k) gives (samples, T + 1, d), y (B, N, k) gives (B, samples, T + 1, d), fp32 on the
    device.  Three launches whatever N: none for the tables (host, float64), one filter, one sampler.  ``A`` must probe as affine
    (``chains.probe_linear``)."""
    model, table, mean, _ = _filter(y, A, sigma, step, burn, chain, device)
    seed = chains._draw_seed() if seed is None else int(seed)
    out = ops.lgss_sample(model, table, mean, samples, seed)
    return out if y.dim() == 3 else out[0]


def enks(y: Tensor, A: Callable[[Tensor], Tensor] = _IDENTITY, sigma: float = 1.0, step: int = 1, members: int = 1024, *,
         lag: Optional[int] = None, inflation: float = 1.0, chain: Optional[chains.LinearGaussian] = None, burn: int = 64,
         seed: Optional[int] = None, device=None, space: str = 'observation') -> Tensor:
    r"""Ensemble-Kalman-smoother samples of p(x_{0:L} | y), (members, T + 1, d) fp32 on the device under the time convention above
    (``chains.enks_fused(...)[:, step:]``): the approximate counterpart of ``posterior``, which it approaches as ``members`` grows.
    ``A`` must probe as an affine selection of state components (``chains.probe_affine``).  ``space='ensemble'`` solves the same
    analysis in ensemble space (``chains.enks_wide``): at most 128 members, ``A`` any callable on the members, not probed."""
    if space not in ('observation', 'ensemble'):
        raise ValueError(f"enks: space={space!r}, expected 'observation' or 'ensemble'")
    chain = make_chain() if chain is None else chain
    if device is None:
        device = y.device if y.is_cuda else torch.device('cuda')
    obs = chains.probe_affine(A, chain, chain.d) if space == 'observation' else None
    if obs is None and space == 'observation':
        raise SdaHipError('enks: A is not an affine selection of state components (each output an affine function of exactly one '
                          'component)')
    x = chain.prior((members,), device=device)
    if burn > 0:
        x = chain.trajectory(x, length=burn, last=True, seed=seed)
    if space == 'ensemble':
        return chains.enks_wide(chain, x, y.to(device), A, sigma, step, lag=lag, inflation=inflation, seed=seed)[:, step:]
    return chains.enks_fused(chain, x, y.to(device), obs, sigma, step, lag=lag, inflation=inflation, seed=seed)[:, step:]


def log_evidence(y: Tensor, A: Callable[[Tensor], Tensor] = _IDENTITY, sigma: float = 1.0, step: int = 1, burn: int = 64, *,
                 chain: Optional[chains.LinearGaussian] = None, device=None) -> Tensor:
    """log p(y), float64 on the device: () for y (N, k), (B,) for y (B, N, k)."""
    logz = _filter(y, A, sigma, step, burn, chain, device)[3]
    return logz if y.dim() == 3 else logz[0]


def log_prior(x: Tensor) -> Tensor:
    r"""sum_i log p(x_{i+1} | x_i) of (..., L, d) trajectories under ``make_chain()``, in torch ops (differentiable)."""
    chain = make_chain()
    return chain.log_prob(x[..., :-1, :], x[..., 1:, :]).sum(dim=-1)


def log_likelihood(y: Tensor, x: Tensor, A: Callable[[Tensor], Tensor] = _IDENTITY, sigma: float = 1.0, step: int = 1) -> Tensor:
    x = x[..., ::step, :]
    log_p = Normal(y, sigma).log_prob(A(x))
    return log_p.sum(dim=(-1, -2))


def posterior_moments(y: Tensor, A: Callable[[Tensor], Tensor] = _IDENTITY, sigma: float = 1.0, step: int = 1, *, burn: int = 64,
                      chain: Optional[chains.LinearGaussian] = None):
    r"""The exact posterior of one observation sequence y (N, k) as (mean (T + 1, d), cov (T + 1, d, d), cross (T, d, d)) with
    cov[i] = Cov(x_i | y) and cross[i] = Cov(x_i, x_{i+1} | y): a Rauch-Tung-Striebel smoother in float64 on the host."""
    chain = make_chain() if chain is None else chain
    H, c = _observation(A, chain)
    Am, b, Q, _, _ = _f64(chain)
    m, P = initial(burn, step, chain)
    y = y.detach().double().cpu()
    N, d = y.shape[0], chain.d
    T = (N - 1) * step
    R = sigma ** 2 * torch.eye(H.shape[0], dtype=torch.float64)
    mf, Pf, Pp = [], [], []
    for i in range(T + 1):
        if i:
            m, P = Am @ m + b, Am @ P @ Am.T + Q
        Pp.append(P)
        if i % step == 0:
            S = H @ P @ H.T + R
            K = torch.linalg.solve(S, H @ P).T
            m = m + K @ (y[i // step] - (H @ m + c))
            IKH = torch.eye(d, dtype=torch.float64) - K @ H
            P = IKH @ P @ IKH.T + K @ R @ K.T
        P = 0.5 * (P + P.T)
        mf.append(m)
        Pf.append(P)
    ms, Ps, cross = [None] * (T + 1), [None] * (T + 1), [None] * T
    ms[T], Ps[T] = mf[T], Pf[T]
    for i in range(T - 1, -1, -1):
        Pn = Am @ Pf[i] @ Am.T + Q
        G = torch.linalg.solve(Pn, Am @ Pf[i]).T
        ms[i] = mf[i] + G @ (ms[i + 1] - (Am @ mf[i] + b))
        Ps[i] = Pf[i] + G @ (Ps[i + 1] - Pn) @ G.T
        Ps[i] = 0.5 * (Ps[i] + Ps[i].T)
        cross[i] = G @ Ps[i + 1]
    empty = torch.empty(0, d, d, dtype=torch.float64)
    return torch.stack(ms), torch.stack(Ps), (torch.stack(cross) if T else empty)


class _ExactEps(torch.autograd.Function):
    """``ops.lgss_score`` with its input gradient: Lambda and the solve commute, so the Jacobian is symmetric and the VJP is the same
    launch on the cotangent around a zero mean."""

    @staticmethod
    def forward(ctx, x, d, T, prec, coef, work):
        ctx.args = (d, T, prec, coef, work)
        return ops.lgss_score(d, T, prec, coef, work, x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        d, T, prec, coef, work = ctx.args
        return ops.lgss_score(d, T, prec, coef, work, g.to(torch.float32).contiguous(), zero_mean=True), None, None, None, None, None


class ExactScore(nn.Module):
    r"""The exact ``eps(x(t), t) = -sigma(t) grad log p(x(t))`` of VP-noised trajectories of a linear-Gaussian chain, as a score module
    ``forward(x, t, c=None)`` over ``(..., length, d)`` that ``VPSDE``, ``PCSampler``, ``GaussianScore`` and ``DPSGaussianScore`` take in
    place of a network.  The trajectory starts at the first observed state of the time convention above (``initial(burn, step)``).

    Per call: ``mu(t), sigma(t)`` on the device (``ops.vp_schedule``, no host read; the schedule is that of the VPSDE given to
    ``bind``, else ``alpha`` / ``eta`` with VPSDE's defaults), one factor launch, one score launch.  ``t`` is one scalar per call.
    Its input gradient is the same score launch on the cotangent (the Jacobian is symmetric), so guidance differentiates through
    it; nothing here reads the device back, so it runs inside ``PCSampler``'s captured step."""

    def __init__(self, chain: chains.LinearGaussian, length: int, burn: int = 64, step: int = 1, alpha: str = 'cos', eta: float = 1e-3):
        super().__init__()
        if length < 1:
            raise ValueError('ExactScore: length >= 1')
        self.chain, self.length, self.burn, self.step = chain, int(length), burn, step
        self.alpha_kind, self.eta = alpha, eta
        A, b, Q, _, _ = _f64(chain)
        m0, P0 = initial(burn, step, chain)
        self._prec_cpu = ops.lgss_score_prec(A, b, Q, m0, P0, self.length - 1)
        self._prec = {}
        self._sde = None

    def bind(self, sde) -> 'ExactScore':
        """Read mu(t), sigma(t) from this VPSDE's schedule (a stock one) instead of ``alpha`` / ``eta``."""
        from ..fused1d import stock_schedule
        if stock_schedule(sde) is None:
            raise SdaHipError('ExactScore.bind: the VPSDE must use a stock schedule (alpha lin / cos / exp, no override)')
        object.__setattr__(self, '_sde', sde)
        return self

    def _schedule(self, t: Tensor) -> Tensor:
        from ..score import _ALPHA_KINDS
        if self._sde is not None:
            from ..fused1d import stock_schedule
            ak, eta, k, kind = stock_schedule(self._sde)
        else:
            ak, eta, kind = _ALPHA_KINDS[self.alpha_kind], self.eta, 0
            k = (0.0, math.acos(math.sqrt(eta)), math.log(eta))[ak]
        return ops.vp_schedule(t.reshape(1), ak, eta, k, kind)

    def prec(self, device) -> Tensor:
        key = ops.kflow_device_key(device)
        p = self._prec.get(key)
        if p is None:
            p = self._prec[key] = self._prec_cpu.to(torch.device(*key))
        return p

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        d, T = self.chain.d, self.length - 1
        ops._dev(x)
        if tuple(x.shape[-2:]) != (self.length, d):
            raise SdaHipError(f'ExactScore: trajectories of shape {tuple(x.shape)}, expected (..., {self.length}, {d})')
        t = torch.as_tensor(t, dtype=torch.float32, device=x.device) if not (torch.is_tensor(t) and t.is_cuda) else t.to(torch.float32)
        if t.numel() != 1:
            raise SdaHipError('ExactScore: one diffusion time per call (the factor is shared by the batch)')
        prec = self.prec(x.device)
        coef = self._schedule(t)
        work = ops.lgss_score_factor(d, T, prec, coef)
        flat = x.reshape(-1, self.length, d)
        return _ExactEps.apply(flat, d, T, prec, coef, work).reshape(x.shape)
