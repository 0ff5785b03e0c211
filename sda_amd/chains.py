r"""Markov chains of the reference (sda/mcs.py:22-241) on the device, and the fused bootstrap particle filter.

``MarkovChain``, ``DiscreteODE``, ``Lorenz63``, ``NoisyLorenz63``, ``Lorenz96`` and ``LotkaVolterra`` keep the reference's
constructor arguments and methods.  ``transition`` and ``trajectory`` of the three built-in systems are ONE launch of
``sda_chain_advance`` (csrc/chain.hip) whatever the length; a user subclass of ``DiscreteODE`` with its own ``f`` -- and any input
that requires grad -- runs the reference's torch-ops ``rk4`` instead (correct, not fused), unless the chain was built with
``grad='device'``: then a float32 device input that requires grad keeps the forward launch and gets its gradient from ONE launch of
``sda_chain_advance_vjp`` (``_ChainAdvance``; ``LAST_CHAIN_GRAD_ROUTE`` records the route of every call).  ``KolmogorovFlow`` is the
incompressible-flow simulator the reference obtains from jax-cfd, here as five launches per sub-step (csrc/kflow.hip: one stencil
kernel and four products with the Hartley matrix on the fp32 matrix cores); see the class.  ``DampedSpring`` (sda/mcs.py:60-82) is a
``LinearGaussian`` chain: one launch of ``sda_lgss_advance`` (csrc/lgss.hip) whatever the length, with the noise convention below; its
exact posterior and exact score live in ``sda_amd.experiments.spring``.

Noise.  The noisy chain draws one 63-bit seed per call from torch's default CPU generator (``torch.manual_seed`` reproduces a
run) unless ``seed=`` is given, and advances a draw counter by the number of transitions, so successive calls never reuse
noise.  The normal added to particle ``r`` at draw ``t`` is row ``r`` of ``ops.randn_rows(.., seed, row0, draw=t)``.

``sda_amd.mcs`` keeps handing out placeholders by default; ``install()`` (or ``sda_amd.install_as_sda(native_chains=True)``)
rebinds the chain names inside that module to the classes of this one.
"""
import abc
import math
from typing import Callable, Optional, Tuple

import torch
from torch import Size, Tensor
from torch.distributions import MultivariateNormal, Normal

from . import ops
from ._lib import CHAIN_MAXOBS, SdaHipError

__all__ = ['MarkovChain', 'DiscreteODE', 'Lorenz63', 'NoisyLorenz63', 'Lorenz96', 'LotkaVolterra', 'KolmogorovFlow', 'LinearGaussian',
           'DampedSpring', 'AffineObservation', 'probe_affine', 'probe_linear', 'bpf_fused', 'enks_fused', 'enks_wide', 'enks_local', 'install']


def _draw_seed() -> int:
    return int(torch.randint(0, 2 ** 63 - 1, (), dtype=torch.int64))


#: gradient route of the last ``transition`` / ``trajectory`` / ``moments`` call of a ``DiscreteODE``: 'device' (the kernel and its
#: adjoint), 'torch' (torch autograd through the torch-ops rk4), or None when the call's input did not require grad
LAST_CHAIN_GRAD_ROUTE = None


class MarkovChain(abc.ABC):
    r"""Abstract first-order time-invariant Markov chain (sda/mcs.py:22-57)."""

    @abc.abstractmethod
    def prior(self, shape: Size = (), *, device=None) -> Tensor:
        r""" x_0 ~ p(x_0) """

    @abc.abstractmethod
    def transition(self, x: Tensor) -> Tensor:
        r""" x_i ~ p(x_i | x_{i-1}) """

    def trajectory(self, x: Tensor, length: int, last: bool = False) -> Tensor:
        r""" (x_1, ..., x_n) ~ \prod_i p(x_i | x_{i-1}) """
        if last:
            for _ in range(length):
                x = self.transition(x)
            return x
        X = []
        for _ in range(length):
            x = self.transition(x)
            X.append(x)
        return torch.stack(X)


class _ChainAdvance(torch.autograd.Function):
    """``ops.chain_advance`` with its adjoint.  Forward is the no-grad launch itself.  Backward is one ``ops.chain_advance_vjp``
    launch over the states each transition started from: the kept frames when the caller asked for them; for ``last`` the forward is
    run again with every frame kept (same seed and first draw, so the noisy chain repeats its noise) into a scratch slab."""

    @staticmethod
    def forward(ctx, flat, model, length, every, seed, draw0):
        m, d = flat.shape
        out = torch.empty((length, m, d) if every else (m, d), device=flat.device, dtype=torch.float32)
        ops.chain_advance(model, flat, out, length, every=every, out_st=m * d, seed=seed, draw0=draw0)
        ctx.model, ctx.length, ctx.every, ctx.seed, ctx.draw0 = model, length, every, seed, draw0
        ctx.save_for_backward(*((flat, out) if every and length > 1 else (flat,)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        flat, *states = ctx.saved_tensors
        states = states[0] if states else None
        length = ctx.length
        if states is None and length > 1:
            m, d = flat.shape
            states = torch.empty(length - 1, m, d, device=flat.device, dtype=torch.float32)
            ops.chain_advance(ctx.model, flat, states, length - 1, every=True, out_st=m * d, seed=ctx.seed, draw0=ctx.draw0)
        g = ops.chain_advance_vjp(ctx.model, flat, states, gout.to(torch.float32).contiguous(), length, ctx.every)
        return g, None, None, None, None, None


class DiscreteODE(MarkovChain):
    r"""Discretized ordinary differential equation (sda/mcs.py:85-122): ``steps`` RK4 sub-steps of ``dt / steps`` per transition.

    ``grad='device'`` (opt-in, keyword only) keeps a float32 device input that requires grad on the kernel: forward is the same
    launch, backward one ``sda_chain_advance_vjp`` launch (first order only).  A user subclass with its own ``f``, Lorenz-96 outside
    4 <= n <= 64, float64 or CPU inputs and the default ``grad='torch'`` differentiate the torch-ops ``rk4``."""

    #: (kernel kind, f of the class the kernel implements); None: torch-ops rk4
    _KERNEL: Optional[Tuple[str, Callable]] = None

    def __init__(self, dt: float = 0.01, steps: int = 1, *, grad: str = 'torch'):
        super().__init__()
        if grad not in ('torch', 'device'):
            raise ValueError(f"{type(self).__name__}: grad={grad!r}, expected 'torch' or 'device'")
        self.grad = grad
        self.dt, self.steps = dt, steps
        self._draw = 0

    @staticmethod
    def rk4(f: Callable[[Tensor], Tensor], x: Tensor, dt: float) -> Tensor:
        k1 = f(x)
        k2 = f(x + dt * k1 / 2)
        k3 = f(x + dt * k2 / 2)
        k4 = f(x + dt * k3)
        return x + dt * (k1 + 2 * k2 + 2 * k3 + k4) / 6

    @abc.abstractmethod
    def f(self, x: Tensor) -> Tensor:
        r""" f(x) = \frac{dx}{dt} """

    # ---- what the kernel needs; the built-in systems fill these in
    def _params(self):
        raise NotImplementedError

    def _noise_std(self) -> float:
        return 0.0

    def _served(self) -> bool:
        """The kernels implement this chain: a built-in system whose ``f`` was not overridden."""
        k = type(self)._KERNEL
        return k is not None and type(self).f is k[1]

    def _fused(self, x: Tensor) -> bool:
        """The kernel serves this call: a built-in system whose ``f`` was not overridden, no autograd through x."""
        return self._served() and not (torch.is_grad_enabled() and x.requires_grad)

    def _grad_route(self, x: Tensor) -> Optional[str]:
        """What carries the gradient of this call, recorded in ``LAST_CHAIN_GRAD_ROUTE``: None if nothing asks for one."""
        global LAST_CHAIN_GRAD_ROUTE
        route = None
        if torch.is_grad_enabled() and x.requires_grad:
            device = self.grad == 'device' and self._served() and x.is_cuda and x.dtype == torch.float32
            route = 'device' if device else 'torch'
        LAST_CHAIN_GRAD_ROUTE = route
        return route

    def model(self):
        kind = type(self)._KERNEL[0]
        d, params = self._params()
        return ops.chain_model(kind, d, self.dt, self.steps, params, self._noise_std())

    def _rk4_transition(self, x: Tensor) -> Tensor:
        for _ in range(self.steps):
            x = self.rk4(self.f, x, self.dt / self.steps)
        return x

    def _advance(self, x: Tensor, length: int, every: bool, seed: Optional[int] = None, *, route: Optional[str] = None) -> Tensor:
        model = self.model()
        if x.shape[-1:] != (model.d,):
            raise SdaHipError(f'{type(self).__name__}: states of shape {tuple(x.shape)}, expected (..., {model.d})')
        batch = x.shape[:-1]
        flat = x.reshape(-1, model.d)
        if flat.stride(-1) != 1:
            flat = flat.contiguous()
        m = flat.shape[0]
        if length < 1 or m < 1:
            raise SdaHipError(f'{type(self).__name__}: length {length}, {m} states')
        draw0 = self._draw
        if model.noise_std > 0:
            seed = _draw_seed() if seed is None else int(seed)
            self._draw += length
        if route == 'device':
            out = _ChainAdvance.apply(flat, model, length, every, seed or 0, draw0)
        else:
            out = torch.empty((length, m, model.d) if every else (m, model.d), device=x.device, dtype=torch.float32)
            ops.chain_advance(model, flat, out, length, every=every, out_st=m * model.d, seed=seed or 0, draw0=draw0)
        return out.reshape((length, *batch, model.d) if every else (*batch, model.d))

    def transition(self, x: Tensor) -> Tensor:
        route = self._grad_route(x)
        if route == 'device' or self._fused(x):
            return self._advance(x, 1, False, route=route)
        return self._rk4_transition(x)

    def trajectory(self, x: Tensor, length: int, last: bool = False) -> Tensor:
        route = self._grad_route(x)
        if (route == 'device' or self._fused(x)) and length >= 1:
            return self._advance(x, length, not last, route=route)
        return super().trajectory(x, length, last)


class Lorenz63(DiscreteODE):
    r"""Lorenz 1963 dynamics (sda/mcs.py:125-172)."""

    def __init__(self, sigma: float = 10.0, rho: float = 28.0, beta: float = 8 / 3, **kwargs):
        super().__init__(**kwargs)
        self.sigma, self.rho, self.beta = sigma, rho, beta

    def prior(self, shape: Size = (), *, device=None) -> Tensor:
        mu = torch.tensor([0.0, 0.0, 25.0])
        sigma = torch.tensor([
            [64.0, 50.0, 0.0],
            [50.0, 81.0, 0.0],
            [0.0, 0.0, 75.0],
        ])
        return MultivariateNormal(mu, sigma).sample(shape).to(device)

    def f(self, x: Tensor) -> Tensor:
        return torch.stack((
            self.sigma * (x[..., 1] - x[..., 0]),
            x[..., 0] * (self.rho - x[..., 2]) - x[..., 1],
            x[..., 0] * x[..., 1] - self.beta * x[..., 2],
        ), dim=-1)

    def _params(self):
        return 3, (self.sigma, self.rho, self.beta)

    @staticmethod
    def preprocess(x: Tensor) -> Tensor:
        mu = x.new_tensor([0.0, 0.0, 25.0])
        sigma = x.new_tensor([8.0, 9.0, 8.6])
        return (x - mu) / sigma

    @staticmethod
    def postprocess(x: Tensor) -> Tensor:
        mu = x.new_tensor([0.0, 0.0, 25.0])
        sigma = x.new_tensor([8.0, 9.0, 8.6])
        return mu + sigma * x


Lorenz63._KERNEL = ('lorenz63', Lorenz63.f)


class NoisyLorenz63(Lorenz63):
    r"""Noisy Lorenz 1963 dynamics (sda/mcs.py:175-185): N(RK4(x), sqrt(dt)) transitions."""

    def _noise_std(self) -> float:
        return self.dt ** 0.5

    def moments(self, x: Tensor) -> Tuple[Tensor, float]:
        route = self._grad_route(x)
        if route == 'device' or self._fused(x):
            model = self.model()
            model.noise_std = 0.0
            flat = x.reshape(-1, 3)
            flat = flat if flat.stride(-1) == 1 else flat.contiguous()
            if route == 'device':
                out = _ChainAdvance.apply(flat, model, 1, False, 0, 0)
            else:
                out = torch.empty_like(flat, memory_format=torch.contiguous_format)
                ops.chain_advance(model, flat, out, 1)
            return out.reshape(x.shape), self.dt ** 0.5
        return self._rk4_transition(x), self.dt ** 0.5

    def transition(self, x: Tensor, *, seed: Optional[int] = None) -> Tensor:
        route = self._grad_route(x)
        if route == 'device' or self._fused(x):
            return self._advance(x, 1, False, seed, route=route)
        return Normal(*self.moments(x)).sample()

    def trajectory(self, x: Tensor, length: int, last: bool = False, *, seed: Optional[int] = None) -> Tensor:
        route = self._grad_route(x)
        if (route == 'device' or self._fused(x)) and length >= 1:
            return self._advance(x, length, not last, seed, route=route)
        return MarkovChain.trajectory(self, x, length, last)

    def log_prob(self, x1: Tensor, x2: Tensor) -> Tensor:
        return Normal(*self.moments(x1)).log_prob(x2).sum(dim=-1)


class Lorenz96(DiscreteODE):
    r"""Lorenz 1996 dynamics (sda/mcs.py:188-211); the kernel serves 4 <= n <= 64."""

    def __init__(self, n: int = 32, F: float = 16.0, **kwargs):
        super().__init__(**kwargs)
        self.n, self.F = n, F

    def prior(self, shape: Size = (), *, device=None) -> Tensor:
        return torch.randn(*shape, self.n).to(device)

    def f(self, x: Tensor) -> Tensor:
        x1, x2, x3 = [torch.roll(x, i, dims=-1) for i in (1, -2, -1)]
        return (x1 - x2) * x3 - x + self.F

    def _params(self):
        return self.n, (self.F,)

    def _served(self) -> bool:
        return 4 <= self.n <= 64 and super()._served()


Lorenz96._KERNEL = ('lorenz96', Lorenz96.f)


class LotkaVolterra(DiscreteODE):
    r"""Lotka-Volterra dynamics (sda/mcs.py:214-241)."""

    def __init__(self, alpha: float = 1.0, beta: float = 1.0, delta: float = 1.0, gamma: float = 1.0, **kwargs):
        super().__init__(**kwargs)
        self.alpha, self.beta = alpha, beta
        self.delta, self.gamma = delta, gamma

    def prior(self, shape: Size = (), *, device=None) -> Tensor:
        return torch.rand(*shape, 2).to(device)

    def f(self, x: Tensor) -> Tensor:
        return torch.stack((
            self.alpha - self.beta * x[..., 1].exp(),
            self.delta * x[..., 0].exp() - self.gamma,
        ), dim=-1)

    def _params(self):
        return 2, (self.alpha, self.beta, self.delta, self.gamma)


LotkaVolterra._KERNEL = ('lotka_volterra', LotkaVolterra.f)


# ---------------------------------------------------------------- Kolmogorov flow
#: gradient route of the last ``KolmogorovFlow.transition`` / ``trajectory`` call: 'device' (the kernels and their adjoint), 'torch'
#: (torch autograd through the torch-ops route), or None when the call's input did not require grad
LAST_KFLOW_GRAD_ROUTE = None


def _kflow_flux(a: Tensor, cm: Tensor, c0: Tensor, cp: Tensor, cpp: Tensor, dh: float) -> Tensor:
    """Van-Leer-limited Lax-Wendroff flux through the face between c0 and cp, advecting velocity a, dh = delta / h."""
    C = a * dh
    d = cp - c0
    pos = a > 0
    low = torch.where(pos, c0, cp)
    high = torch.where(pos, c0 + 0.5 * (1 - C) * d, cp - 0.5 * (1 + C) * d)
    num = torch.where(pos, c0 - cm, cpp - cp)
    nz = d != 0
    r = torch.where(nz, num / torch.where(nz, d, torch.ones_like(d)), torch.zeros_like(d))
    ar = r.abs()
    phi = (r + ar) / (1 + ar)
    return (low + phi * (high - low)) * a


def _shift(a: Tensor, di: int, dj: int) -> Tensor:
    """a[i + di, j + dj] on the periodic grid."""
    return torch.roll(a, (-di, -dj), (-2, -1))


class _KflowAdvance(torch.autograd.Function):
    """``ops.kflow_advance`` with its adjoint.  Forward keeps every frame (the caller's own result when it asked for them, the
    checkpoints otherwise); backward walks the transitions last to first, one ``ops.kflow_transition_vjp`` each, and adds the
    cotangent of a kept frame as it passes it.  Memory: the frames plus one transition's slab of sub-step states."""

    @staticmethod
    def forward(ctx, x, model, length, last):
        frames = ops.kflow_advance(model, x, length, every=length > 1 or not last)
        ctx.model, ctx.length, ctx.last = model, length, last
        ctx.save_for_backward(*((x, frames) if length > 1 else (x,)))      # one transition needs its input alone
        if not last:
            return frames
        return frames[-1] if length > 1 else frames

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, *frames = ctx.saved_tensors
        frames = frames[0] if frames else None
        length, last = ctx.length, ctx.last
        gout = gout.to(torch.float32)
        g = gout if last else gout[length - 1]
        for t in range(length - 1, -1, -1):
            g = ops.kflow_transition_vjp(ctx.model, frames[t - 1] if t else x, g)
            if t and not last:
                g = g + gout[t - 1]
        return g, None, None, None


class KolmogorovFlow(MarkovChain):
    r"""2-D incompressible flow with Kolmogorov forcing (sda/mcs.py:244-338) on the device.

    The reference only calls jax-cfd, so the scheme here is this project's restatement of ``semi_implicit_navier_stokes`` with its
    defaults (tests/kflow_ref.py): faithful, not pinned to a reference output, and the random stream of
    ``prior`` is this package's Philox (``ops.randn_rows`` keyed on (seed, row)), not jax's.

    State ``(..., 2, size, size)`` fp32: u, v on a staggered periodic grid, axis -2 is x.  A transition is ``steps`` sub-steps;
    ``transition`` and ``trajectory`` queue every launch (five per sub-step, csrc/kflow.hip) and read nothing back, and
    ``trajectory`` writes each kept frame straight into its slab.  The kernels serve ``size % 16 == 0, 16 <= size <= 512``; other
    sizes and inputs that require grad take the same scheme in torch ops (``_torch_substep``: ``torch.roll`` and ``torch.fft``,
    differentiable).  A CPU tensor at a served size raises, as the Lorenz chains do.

    ``grad='device'`` (opt-in) sends float32 HIP inputs that require grad at a served size through the kernels as well: forward is
    ``ops.kflow_advance`` itself (bitwise the no-grad values), backward recomputes one transition's sub-step states at a time and
    runs them backwards with the projection (its own transpose) and the explicit terms' VJP kernel.  First order only.
    ``LAST_KFLOW_GRAD_ROUTE`` records the route a call took."""

    def __init__(self, size: int = 256, dt: float = 0.01, reynolds: int = 1e3, *, grad: str = 'torch'):
        super().__init__()
        if grad not in ('torch', 'device'):
            raise ValueError(f"KolmogorovFlow: grad={grad!r}, expected 'torch' or 'device'")
        self.grad = grad
        self.size, self.dt, self.reynolds = int(size), dt, reynolds
        h = 2 * math.pi / self.size
        nu = 1 / reynolds
        dt_min = min(0.5 * h / 5.0, h * h / (4 * nu))
        self.steps = 1 if dt_min > dt else math.ceil(dt / dt_min)
        # the fp32 values the kernels are handed; every route and precision uses the same two numbers
        self.delta = torch.tensor(dt / self.steps, dtype=torch.float32).item()
        self.nu = torch.tensor(nu, dtype=torch.float32).item()
        self._kernel_size = self.size % 16 == 0 and 16 <= self.size <= 512
        self._models, self._filters = {}, {}

    # ---- routes
    def _fused(self, x: Tensor) -> bool:
        return self._kernel_size and not (torch.is_grad_enabled() and x.requires_grad)

    def model(self, device):
        key = ops.kflow_device_key(device)
        m = self._models.get(key)
        if m is None:
            m = self._models[key] = ops.kflow_model(self.size, self.steps, self.delta, self.nu, torch.device(*key))
        return m

    def _check(self, x: Tensor) -> None:
        if tuple(x.shape[-3:]) != (2, self.size, self.size):
            raise SdaHipError(f'KolmogorovFlow: states of shape {tuple(x.shape)}, expected (..., 2, {self.size}, {self.size})')

    # ---- the scheme in torch ops
    def _torch_project(self, x: Tensor) -> Tensor:
        n = self.size
        h = 2 * math.pi / n
        u, v = x[..., 0, :, :], x[..., 1, :, :]
        div = ((u - _shift(u, -1, 0)) + (v - _shift(v, 0, -1))) / h
        inv = ops.kflow_solve_tables(n, x.device, x.dtype)[0]
        q = torch.fft.ifft2(torch.fft.fft2(div) * inv).real
        return torch.stack((u - (_shift(q, 1, 0) - q) / h, v - (_shift(q, 0, 1) - q) / h), dim=-3)

    def _torch_explicit(self, x: Tensor) -> Tensor:
        n = self.size
        h = 2 * math.pi / n
        delta, nu, dh = self.delta, self.nu, self.delta / h
        u, v = x[..., 0, :, :], x[..., 1, :, :]

        def adv(c, ax, ay):
            fx = _kflow_flux(ax, _shift(c, -1, 0), c, _shift(c, 1, 0), _shift(c, 2, 0), dh)
            fy = _kflow_flux(ay, _shift(c, 0, -1), c, _shift(c, 0, 1), _shift(c, 0, 2), dh)
            return ((fx - _shift(fx, -1, 0)) + (fy - _shift(fy, 0, -1))) / h

        def lap(c):
            return ((((_shift(c, 1, 0) + _shift(c, -1, 0)) + _shift(c, 0, 1)) + _shift(c, 0, -1)) - 4 * c) / (h * h)

        forcing = ops.kflow_solve_tables(n, x.device, x.dtype)[1]
        au = adv(u, 0.5 * (u + _shift(u, 1, 0)), 0.5 * (v + _shift(v, 1, 0)))
        av = adv(v, 0.5 * (u + _shift(u, 0, 1)), 0.5 * (v + _shift(v, 0, 1)))
        us = u + delta * ((nu * lap(u) - au) + (forcing - 0.1 * u))
        vs = v + delta * ((nu * lap(v) - av) + (-0.1 * v))
        return torch.stack((us, vs), dim=-3)

    def _torch_substep(self, x: Tensor) -> Tensor:
        """One sub-step in torch ops: the fallback of the kernels, differentiable, and the timing baseline."""
        return self._torch_project(self._torch_explicit(x))

    def _torch_transition(self, x: Tensor) -> Tensor:
        for _ in range(self.steps):
            x = self._torch_substep(x)
        return x

    # ---- MarkovChain
    def _filter(self, device) -> Tensor:
        """g(|k|) of jax-cfd's filtered_velocity_field (peak wavenumber 4): a log-normal in |k|, 0 at k = 0; (size, size)."""
        key = ops.kflow_device_key(device)
        device = torch.device(*key)
        g = self._filters.get(key)
        if g is None:
            n = self.size
            k = torch.arange(n, dtype=torch.float64)
            k = torch.where(k > n // 2, k - n, k)
            kk = (k[:, None] ** 2 + k[None, :] ** 2).sqrt()
            kk[0, 0] = 1.0
            lk = kk.log()
            g = torch.exp(-(math.log(4.0) + 0.25 - lk) ** 2 / (2 * 0.25) - lk) / math.sqrt(2 * math.pi * 0.25)
            g[0, 0] = 0.0
            g = self._filters[key] = g.float().to(device)
        return g

    def prior(self, shape: Size = (), *, device=None, seed: Optional[int] = None) -> Tensor:
        r"""Filtered unit normal noise, then three rounds of {project; scale the largest speed to 3}.  The noise of field ``r`` is
        row ``r`` of ``ops.randn_rows(.., seed, 0)``; ``seed`` defaults to one draw from torch's CPU generator.  ``device`` defaults
        to the current HIP device (the generator has no CPU form).  The filter and the projection run on the kernels at a served
        size; the rescaling is three small torch reductions."""
        shape = Size(shape)
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        seed = _draw_seed() if seed is None else int(seed)
        n = self.size
        if shape.numel() == 0:
            return torch.empty(*shape, 2, n, n, device=device, dtype=torch.float32)
        z = torch.empty(shape.numel(), 2, n, n, device=device, dtype=torch.float32)
        ops.randn_rows(z, seed, 0)
        g = self._filter(device)
        if self._kernel_size:
            x = ops.kflow_hartley(ops.kflow_hartley(z, g))
        else:
            x = torch.fft.ifft2(torch.fft.fft2(z) * g).real
        for _ in range(3):
            x = ops.kflow_project(self.model(device), x) if self._kernel_size else self._torch_project(x)
            speed = (x[:, 0] ** 2 + x[:, 1] ** 2).amax(dim=(-2, -1)).sqrt()
            # a field that is zero everywhere has no direction to scale: it stays zero
            x = x * torch.where(speed > 0, 3.0 / speed, torch.zeros_like(speed))[:, None, None, None]
        return x.reshape(*shape, 2, n, n)

    def _grad_route(self, x: Tensor) -> Optional[str]:
        """What carries the gradient of this call, recorded in ``LAST_KFLOW_GRAD_ROUTE``: None if nothing asks for one."""
        global LAST_KFLOW_GRAD_ROUTE
        route = None
        if torch.is_grad_enabled() and x.requires_grad:
            served = self.grad == 'device' and self._kernel_size and x.is_cuda and x.dtype == torch.float32
            route = 'device' if served else 'torch'
        LAST_KFLOW_GRAD_ROUTE = route
        return route

    def transition(self, x: Tensor) -> Tensor:
        self._check(x)
        if self._grad_route(x) == 'device':
            return _KflowAdvance.apply(x, self.model(x.device), 1, True)
        if self._fused(x):
            return ops.kflow_advance(self.model(x.device), x, 1) if x.is_cuda else ops._dev(x)
        return self._torch_transition(x)

    def trajectory(self, x: Tensor, length: int, last: bool = False) -> Tensor:
        self._check(x)
        if self._grad_route(x) == 'device' and length >= 1:
            return _KflowAdvance.apply(x, self.model(x.device), length, last)
        if self._fused(x) and length >= 1:
            return ops.kflow_advance(self.model(x.device), x, length, every=not last) if x.is_cuda else ops._dev(x)
        return super().trajectory(x, length, last)

    @staticmethod
    def coarsen(x: Tensor, r: int = 2) -> Tensor:
        return _mcs()._coarsen(x, r)

    @staticmethod
    def upsample(x: Tensor, r: int = 2, mode: str = 'bilinear') -> Tensor:
        return _mcs()._upsample(x, r, mode)

    @staticmethod
    def vorticity(x: Tensor) -> Tensor:
        return _mcs()._vorticity(x)


def _mcs():
    """``sda_amd.mcs``, loaded on first use (it probes for a user's own sda/mcs.py): its torch-only static helpers are the ones
    ``KolmogorovFlow`` hands out."""
    import importlib
    return importlib.import_module(__package__ + '.mcs')


# ---------------------------------------------------------------- linear-Gaussian chains
class LinearGaussian(MarkovChain):
    r"""x_0 ~ N(m0, S0), x_{i+1} = A x_i + b + w_i, w_i ~ N(0, Q) with Q symmetric positive definite and 1 <= d <= 8.

    ``transition`` and ``trajectory`` are ONE launch of ``sda_lgss_advance`` whatever the length (fp32; the normal added to state
    ``r`` at draw ``t`` is ``Lq`` times row ``r`` of ``ops.randn_rows(.., seed, 0, draw=t)``, ``Lq`` the Cholesky factor of Q), with
    the seed and draw counter of ``NoisyLorenz63``.  An input that requires grad takes the reference's torch expression; a CPU
    tensor raises, as for the other built-in chains."""

    def __init__(self, A, b, Q, m0, S0):
        super().__init__()
        as32 = lambda v: torch.as_tensor(v, dtype=torch.float32).detach().clone().cpu()
        self.A, self.b, self.Sigma_x = as32(A), as32(b), as32(Q)
        self.mu_0, self.Sigma_0 = as32(m0), as32(S0)
        self.d = self.b.numel()
        self._model = ops.lgss_model(self.A.double(), self.b.double(), self.Sigma_x.double())
        self._draw = 0

    def model(self):
        return self._model

    def prior(self, shape: Size = (), *, device=None) -> Tensor:
        return MultivariateNormal(self.mu_0, self.Sigma_0).sample(shape).to(device)

    def _fused(self, x: Tensor) -> bool:
        return not (torch.is_grad_enabled() and x.requires_grad)

    def moments(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        r"""Mean and covariance of p(x_{i+1} | x_i = x), in torch ops on x's device."""
        return x @ self.A.to(x).T + self.b.to(x), self.Sigma_x.to(x)

    def _advance(self, x: Tensor, length: int, every: bool, seed: Optional[int] = None) -> Tensor:
        d = self.d
        if x.shape[-1:] != (d,):
            raise SdaHipError(f'{type(self).__name__}: states of shape {tuple(x.shape)}, expected (..., {d})')
        ops._dev(x)
        batch = x.shape[:-1]
        flat = x.reshape(-1, d)
        if flat.stride(-1) != 1:
            flat = flat.contiguous()
        m = flat.shape[0]
        if length < 1 or m < 1:
            raise SdaHipError(f'{type(self).__name__}: length {length}, {m} states')
        draw0 = self._draw
        seed = _draw_seed() if seed is None else int(seed)
        self._draw += length
        out = torch.empty((length, m, d) if every else (m, d), device=x.device, dtype=torch.float32)
        ops.lgss_advance(self._model, flat, out, length, every=every, out_st=m * d, seed=seed, draw0=draw0)
        return out.reshape((length, *batch, d) if every else (*batch, d))

    def transition(self, x: Tensor, *, seed: Optional[int] = None) -> Tensor:
        if self._fused(x):
            return self._advance(x, 1, False, seed)
        return MultivariateNormal(*self.moments(x)).sample()

    def trajectory(self, x: Tensor, length: int, last: bool = False, *, seed: Optional[int] = None) -> Tensor:
        if self._fused(x) and length >= 1:
            return self._advance(x, length, not last, seed)
        return MarkovChain.trajectory(self, x, length, last)

    def log_prob(self, x1: Tensor, x2: Tensor) -> Tensor:
        return MultivariateNormal(*self.moments(x1)).log_prob(x2)


class DampedSpring(LinearGaussian):
    r"""Linearized dynamics of a mass attached to a spring, subject to wind and drag (sda/mcs.py:60-82)."""

    def __init__(self, dt: float = 0.01):
        self.dt = dt
        super().__init__(
            A=torch.tensor([
                [1.0, dt, dt**2 / 2, 0.0],
                [0.0, 1.0, dt, 0.0],
                [-0.5, -0.1, 0.0, 0.2],
                [0.0, 0.0, 0.0, 0.99],
            ]),
            b=torch.tensor([0.0, 0.0, 0.0, 0.0]),
            Q=torch.tensor([0.1, 0.1, 0.1, 1.0]).diag() * dt,
            m0=torch.tensor([1.0, 0.0, 0.0, 0.0]),
            S0=torch.tensor([1.0, 1.0, 1.0, 1.0]).diag(),
        )


# ---------------------------------------------------------------- observation operators the fused filter understands
class AffineObservation:
    r"""A(x) = (x[..., index] - shift) / scale: each output is an affine function of ONE state component."""

    def __init__(self, index, shift, scale):
        self.index = [int(i) for i in index]
        self.shift = [float(s) for s in shift]
        self.scale = [float(s) for s in scale]
        if not (1 <= len(self.index) <= CHAIN_MAXOBS) or len(self.shift) != len(self.index) or len(self.scale) != len(self.index):
            raise ValueError('AffineObservation: index, shift and scale are equally long lists of 1 to 64 entries')
        if any(s == 0 for s in self.scale):
            raise ValueError('AffineObservation: zero scale')

    def __call__(self, x: Tensor) -> Tensor:
        return (x[..., self.index] - x.new_tensor(self.shift)) / x.new_tensor(self.scale)

    def __repr__(self):
        return f'AffineObservation(index={self.index}, shift={self.shift}, scale={self.scale})'


def probe_affine(A: Callable[[Tensor], Tensor], chain: MarkovChain, d: int, rtol: float = 1e-6) -> Optional[AffineObservation]:
    """Recover an AffineObservation from a callable, or None: evaluate A at 0 and at the d unit vectors (float64, host), require
    every output to depend on exactly one component, then confirm A(x) = the recovered map on 64 prior-scale random states to
    `rtol` of the largest output.  torch's global generator is left as it was."""
    if isinstance(A, AffineObservation):
        return A
    try:
        with torch.no_grad():
            b = A(torch.zeros(d, dtype=torch.float64))
            if b.dim() != 1 or not 1 <= b.numel() <= min(d, CHAIN_MAXOBS) or not b.is_floating_point():
                return None
            cols = A(torch.eye(d, dtype=torch.float64))
            if cols.shape != (d, b.numel()):
                return None
            M = (cols - b).T                                  # (k, d): output r = sum_c M[r, c] x[c] + b[r]
            if not (torch.isfinite(M).all() and torch.isfinite(b).all()) or ((M != 0).sum(dim=1) != 1).any():
                return None
            index = M.abs().argmax(dim=1)
            gain = M[torch.arange(len(index)), index]
            obs = AffineObservation(index.tolist(), (-b / gain).tolist(), (1 / gain).tolist())
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(0)
                x = chain.prior((64,)).double().cpu()
            got, want = A(x), obs(x)
            if got.shape != want.shape or not ((got - want).abs().max() <= rtol * want.abs().max().clamp_min(1e-300)):
                return None
            return obs
    except Exception:  # noqa: BLE001 -- a callable that cannot take these inputs is simply not recognised
        return None


def probe_linear(A: Callable[[Tensor], Tensor], chain: MarkovChain, d: int, rtol: float = 1e-6) -> Optional[Tuple[Tensor, Tensor]]:
    """Recover (H, c), float64 (k, d) and (k,), with A(x) = H x + c from a callable, or None: evaluate A at 0 and at the d unit vectors
    (float64, host), then confirm on 64 prior-scale random states to `rtol` of the largest output.  Unlike ``probe_affine`` an output
    may depend on every component (a dense H); 1 <= k <= 8.  torch's global generator is left as it was."""
    try:
        with torch.no_grad():
            c = A(torch.zeros(d, dtype=torch.float64))
            if c.dim() != 1 or not 1 <= c.numel() <= 8 or not c.is_floating_point():
                return None
            cols = A(torch.eye(d, dtype=torch.float64))
            if cols.shape != (d, c.numel()):
                return None
            H = (cols - c).T.contiguous().double()
            c = c.double()
            if not (torch.isfinite(H).all() and torch.isfinite(c).all()):
                return None
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(0)
                x = chain.prior((64,)).double().cpu()
            got, want = A(x), x @ H.T + c
            if got.shape != want.shape or not ((got - want).abs().max() <= rtol * want.abs().max().clamp_min(1e-300)):
                return None
            return H, c
    except Exception:  # noqa: BLE001 -- a callable that cannot take these inputs is simply not recognised
        return None


def bpf_fused(chain: DiscreteODE, x: Tensor, y: Tensor, obs: AffineObservation, sigma: float, step: int = 1, *,
              seed: Optional[int] = None, record: Optional[dict] = None) -> Tensor:
    r"""Bootstrap particle filter (sda/utils.py:168-200) with ``chain.transition`` and the Gaussian likelihood
    N(y_i; obs(x), sigma): per observation ONE advance launch (``step`` transitions read through the previous ancestors, the
    log-weights of the last state), one cdf launch and one resample launch; one traceback at the end.  x (M, d) initial
    particles, y (N, k); returns (M, N step + 1, d).  Raises SdaHipError if an observation leaves no particle with weight.
    ``record``: a dict that receives the un-resampled states ``S`` and the ancestors ``anc`` (tests)."""
    ops._dev(x)
    model = chain.model()
    m, d = x.shape
    n = len(y)
    y = y.to(device=x.device, dtype=torch.float32).reshape(n, -1).contiguous()
    if y.shape[1] != len(obs.index) or n < 1 or step < 1:
        raise SdaHipError(f'bpf_fused: {tuple(y.shape)} observations for {len(obs.index)} observed components, step {step}')
    seed = _draw_seed() if seed is None else int(seed)
    draw0 = chain._draw
    chain._draw += n * step
    dev = x.device
    S = torch.empty(n * step + 1, m, d, device=dev, dtype=torch.float32)
    S[0] = x
    anc = torch.empty(n, m, device=dev, dtype=torch.int32)
    status = torch.zeros(n, device=dev, dtype=torch.int32)
    logw = torch.empty(m, device=dev, dtype=torch.float32)
    pmax = torch.empty(ops._lib.load().sda_bpf_logweights_blocks(m), device=dev, dtype=torch.float32)
    w = torch.empty(m, device=dev, dtype=torch.float32)
    cdf = torch.empty(m, device=dev, dtype=torch.float64)
    o = ops.chain_obs(obs.index, obs.shift, obs.scale, sigma, y[0])
    for k in range(n):
        o.y = y[k].data_ptr()
        ops.chain_advance(model, S[k * step], S[k * step + 1:], step, every=True, out_st=m * d, anc=anc[k - 1] if k else None,
                          seed=seed, draw0=draw0 + k * step, obs=o, logw=logw, pmax=pmax)
        ops.bpf_cdf(logw, pmax, w=w, cdf=cdf, status=status[k:k + 1], check=False)
        ops.bpf_resample(cdf, seed, k, anc[k])
    out = ops.bpf_traceback(S, anc, step)
    ops.bpf_check(status)                                    # the one read-back of the filter
    if record is not None:
        record.update(S=S, anc=anc, seed=seed, draw0=draw0)
    return out


def enks_fused(chain: MarkovChain, x: Tensor, y: Tensor, obs: AffineObservation, sigma: float, step: int = 1, *,
               lag: Optional[int] = None, inflation: float = 1.0, seed: Optional[int] = None, record: Optional[dict] = None) -> Tensor:
    r"""Stochastic (perturbed-observation) ensemble Kalman smoother with ``chain``'s transitions and the Gaussian likelihood
    N(y_i; obs(x), sigma): per observation ONE forecast launch (``step`` transitions written straight into the time-major
    ensemble), one gain launch and one update launch over the smoothing window (csrc/enks.hip; the five steps are in
    include/sda_hip.h).  x (M, d) initial members, y (N, k); returns (M, N step + 1, d).  Observation i sits at time (i + 1) step;
    its analysis updates the times lo .. (i + 1) step with lo = 0, or max(0, (i + 1 - lag) step) when ``lag`` (in observations) is
    given; ``lag=0`` is the ensemble Kalman filter.  ``inflation`` scales the forecast anomalies of the observed time.

    The forecast of a served ``DiscreteODE`` is ``ops.chain_advance`` with ``bpf_fused``'s draw bookkeeping; any other chain
    (``DampedSpring``) forecasts with ``chain.trajectory``.  The perturbation of member j at observation i is row j of
    ``ops.randn_rows(.., seed ^ 0x454E4B53, 0, draw=i)``.  One read-back, at the end: raises SdaHipError if an innovation
    covariance had no Cholesky factor.  ``record``: a dict that receives, per analysis, the ensemble before it (``S``), ``a``,
    ``z``, and the status words (tests and small shapes only: every entry is a copy)."""
    ops._dev(x)
    if x.dim() != 2:
        raise SdaHipError(f'enks_fused: members of shape {tuple(x.shape)}, expected (M, d)')
    m, d = x.shape
    n = len(y)
    y = y.to(device=x.device, dtype=torch.float32).reshape(n, -1).contiguous()
    if y.shape[1] != len(obs.index) or n < 1 or step < 1 or m < 2 or (lag is not None and lag < 0):
        raise SdaHipError(f'enks_fused: {tuple(y.shape)} observations for {len(obs.index)} observed components, {m} members, step '
                          f'{step}, lag {lag}')
    served = isinstance(chain, DiscreteODE) and chain._served()
    seed = _draw_seed() if seed is None else int(seed)
    dev = x.device
    S = torch.empty(n * step + 1, m, d, device=dev, dtype=torch.float32)
    S[0] = x
    if served:
        model = chain.model()
        if model.d != d:
            raise SdaHipError(f'enks_fused: members of shape {tuple(x.shape)} for a {model.d}-component chain')
        draw0 = chain._draw
        chain._draw += n * step
    k = len(obs.index)
    a, z, work = (torch.empty(k, m, device=dev, dtype=torch.float32) for _ in range(3))
    status = torch.zeros(n, device=dev, dtype=torch.int32)
    o = ops.chain_obs(obs.index, obs.shift, obs.scale, sigma, y[0])
    if record is not None:
        record.update(S=[], a=[], z=[], seed=seed)
    for i in range(n):
        t = (i + 1) * step
        if served:
            ops.chain_advance(model, S[i * step], S[i * step + 1:], step, every=True, out_st=m * d, seed=seed, draw0=draw0 + i * step)
        elif isinstance(chain, (LinearGaussian, NoisyLorenz63)):
            S[i * step + 1:t + 1] = chain.trajectory(S[i * step], step, seed=seed)
        else:
            S[i * step + 1:t + 1] = chain.trajectory(S[i * step], step)
        lo = 0 if lag is None else max(0, t - lag * step)
        o.y = y[i].data_ptr()
        if record is not None:
            record['S'].append(S.clone())
        ops.enks_gain(S, t, o, inflation=inflation, seed=seed, draw=i, a=a, z=z, work=work, status=status[i:i + 1])
        ops.enks_update(S, lo, t, a, z, inflation=inflation)
        if record is not None:
            record['a'].append(a.clone())
            record['z'].append(z.clone())
    if record is not None:
        record.update(status=status.clone())
    ops.enks_check(status)                                   # the one read-back of the smoother
    return S.permute(1, 0, 2).contiguous()


def enks_wide(chain: MarkovChain, x: Tensor, y: Tensor, A: Callable[[Tensor], Tensor], sigma: float, step: int = 1, *,
              lag: Optional[int] = None, inflation: float = 1.0, seed: Optional[int] = None, record: Optional[dict] = None) -> Tensor:
    r"""``enks_fused``'s smoother solved in ensemble space (csrc/enks_wide.hip; the arithmetic is in include/sda_hip.h): for wide
    states and M <= 128 members, with ``A`` ANY callable from (M, \*event) members to (M, \*obs) observed values, applied with
    torch or the ``observe`` operators.  x (M, \*event) initial members, y (N, \*obs); returns (M, N step + 1, \*event).  Time
    convention, ``lag`` and ``inflation`` are ``enks_fused``'s, and the perturbation of member j at observation i is the same row j
    of ``ops.randn_rows(.., seed ^ 0x454E4B53, 0, draw=i)``.

    Every forecast is ``chain.trajectory``; per analysis four launches (five with inflation) beside ``A`` itself.  One read-back, at
    the end: raises SdaHipError if an analysis had no Cholesky factor or a non-finite transform.  ``record``: a dict that receives,
    per analysis, the ensemble before it (``S``, time-major and flattened to (time, M, d)), ``H``, ``W``, and the status words (tests
    and small shapes only: every entry is a copy)."""
    ops._dev(x)
    if x.dim() < 2:
        raise SdaHipError(f'enks_wide: members of shape {tuple(x.shape)}, expected (M, *event)')
    m, event = x.shape[0], tuple(x.shape[1:])
    n = len(y)
    y = y.to(device=x.device, dtype=torch.float32).reshape(n, -1).contiguous()
    k = y.shape[1]
    if n < 1 or k < 1 or step < 1 or not 2 <= m <= ops.ENKW_MAX_M or (lag is not None and lag < 0):
        raise SdaHipError(f'enks_wide: {tuple(y.shape)} observations, {m} members (2 .. {ops.ENKW_MAX_M} are served), step {step}, '
                          f'lag {lag}')
    seed = _draw_seed() if seed is None else int(seed)
    kw = {'seed': seed} if isinstance(chain, (LinearGaussian, NoisyLorenz63)) else {}
    dev = x.device
    S = torch.empty((n * step + 1, m) + event, device=dev, dtype=torch.float32)
    S[0] = x
    flat = S.view(n * step + 1, m, -1)
    Y, D, eps = (torch.empty(m, k, device=dev, dtype=torch.float32) for _ in range(3))
    part = torch.empty(ops._lib.load().sda_enkw_gram_doubles(m, k), device=dev, dtype=torch.float64)
    work = torch.empty(m * m, device=dev, dtype=torch.float64)
    W = torch.empty(m, m, device=dev, dtype=torch.float32)
    status = torch.zeros(n, device=dev, dtype=torch.int32)
    if record is not None:
        record.update(S=[], H=[], W=[], seed=seed)
    for i in range(n):
        t = (i + 1) * step
        S[i * step + 1:t + 1] = chain.trajectory(S[i * step], step, **kw)
        lo = 0 if lag is None else max(0, t - lag * step)
        if record is not None:
            record['S'].append(flat.clone())
        ops.enkw_inflate(flat, t, inflation)
        H = A(S[t])
        if H.shape[0] != m or H.numel() != m * k:
            raise SdaHipError(f'enks_wide: A gave {tuple(H.shape)} for {m} members and observations of {k} values')
        H = H.to(torch.float32).reshape(m, k).contiguous()
        ops.enkw_prepare(H, y[i], sigma, seed=seed, draw=i, Y=Y, D=D, eps=eps)
        ops.enkw_gram(Y, D, part=part)
        ops.enkw_solve(part, m, k, sigma, W=W, status=status[i:i + 1], work=work)
        ops.enkw_transform(flat, lo, t, W)
        if record is not None:
            record['H'].append(H.clone())
            record['W'].append(W.clone())
    if record is not None:
        record.update(status=status.clone())
    ops.enks_check(status)                                   # the one read-back of the smoother
    return S.transpose(0, 1).contiguous()


def enks_local(chain: MarkovChain, x: Tensor, y: Tensor, A: Callable[[Tensor], Tensor], sigma: float, step: int = 1, *,
               positions, radius: float, block, lag: Optional[int] = None, inflation: float = 1.0, seed: Optional[int] = None,
               record: Optional[dict] = None) -> Tensor:
    r"""``enks_wide``'s smoother with the analysis LOCALISED by domain (csrc/enks_local.hip; the arithmetic is in
    include/sda_hip.h): the event of ``x`` is a periodic grid (C, Hg, Wg), or a ring (n,), cut into blocks of ``block`` points;
    every block solves its own M x M system over the observed values within ``2 radius`` grid points of its centre, each weighted
    by the Gaspari-Cohn function of its distance, and updates its own components.  ``positions`` (k, 2) are the (row, col) of the
    observed values in ``A``'s flattened output order ((k,) on a ring; ``observe.positions(A, event)`` gives them for the operators
    whose outputs sit on the grid); ``radius=float('inf')`` with one block is ``enks_wide``'s analysis.  Signature otherwise, time
    convention, ``lag``, ``inflation``, perturbation stream and return shape are ``enks_wide``'s; M <= 128.

    The plan is built once (``ops.enkl_plan``); per analysis four launches (five with inflation) beside ``A`` itself.  One
    read-back, at the end: raises SdaHipError if a block of an analysis had no Cholesky factor or a non-finite transform (that
    block alone was left untouched).  ``record`` receives what ``enks_wide``'s does, with ``W`` of shape (nblk, M, M) and the
    status words (N, nblk), and the ``plan``."""
    ops._dev(x)
    if x.dim() not in (2, 4):
        raise SdaHipError(f'enks_local: members of shape {tuple(x.shape)}, expected (M, C, Hg, Wg) or (M, n)')
    m, event = x.shape[0], tuple(x.shape[1:])
    n = len(y)
    y = y.to(device=x.device, dtype=torch.float32).reshape(n, -1).contiguous()
    k = y.shape[1]
    if n < 1 or k < 1 or step < 1 or not 2 <= m <= ops.ENKW_MAX_M or (lag is not None and lag < 0):
        raise SdaHipError(f'enks_local: {tuple(y.shape)} observations, {m} members (2 .. {ops.ENKW_MAX_M} are served), step {step}, '
                          f'lag {lag}')
    plan = ops.enkl_plan(event, positions, radius, block, device=x.device)
    if plan.k != k:
        raise SdaHipError(f'enks_local: {plan.k} positions for observations of {k} values')
    seed = _draw_seed() if seed is None else int(seed)
    kw = {'seed': seed} if isinstance(chain, (LinearGaussian, NoisyLorenz63)) else {}
    dev = x.device
    S = torch.empty((n * step + 1, m) + event, device=dev, dtype=torch.float32)
    S[0] = x
    flat = S.view(n * step + 1, m, -1)
    Y, D, eps = (torch.empty(m, k, device=dev, dtype=torch.float32) for _ in range(3))
    W = torch.empty(plan.nblk, m, m, device=dev, dtype=torch.float32)
    status = torch.zeros(n, plan.nblk, device=dev, dtype=torch.int32)
    if record is not None:
        record.update(S=[], H=[], W=[], seed=seed, plan=plan)
    for i in range(n):
        t = (i + 1) * step
        S[i * step + 1:t + 1] = chain.trajectory(S[i * step], step, **kw)
        lo = 0 if lag is None else max(0, t - lag * step)
        if record is not None:
            record['S'].append(flat.clone())
        ops.enkw_inflate(flat, t, inflation)
        H = A(S[t])
        if H.shape[0] != m or H.numel() != m * k:
            raise SdaHipError(f'enks_local: A gave {tuple(H.shape)} for {m} members and observations of {k} values')
        H = H.to(torch.float32).reshape(m, k).contiguous()
        ops.enkw_prepare(H, y[i], sigma, seed=seed, draw=i, Y=Y, D=D, eps=eps)
        ops.enkl_weights(plan, Y, D, sigma, W=W, status=status[i])
        ops.enkl_transform(plan, flat, lo, t, W)
        if record is not None:
            record['H'].append(H.clone())
            record['W'].append(W.clone())
    if record is not None:
        record.update(status=status.clone())
    ops.enkl_check(status)                                   # the one read-back of the smoother
    return S.transpose(0, 1).contiguous()


def install() -> None:
    """Rebind the chain names inside ``sda_amd.mcs`` (= ``sda.mcs`` after ``install_as_sda``) to the classes of this module;
    call it before a driver's ``from sda.mcs import *``."""
    import importlib
    mcs = importlib.import_module(__package__ + '.mcs')
    for name in ('MarkovChain', 'DiscreteODE', 'Lorenz63', 'NoisyLorenz63', 'Lorenz96', 'LotkaVolterra', 'KolmogorovFlow', 'DampedSpring'):
        setattr(mcs, name, globals()[name])
    mcs.SOURCE = __name__
