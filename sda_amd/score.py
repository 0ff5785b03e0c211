r"""Score modules -- MI355X host-side mirror of the reference's ``sda/score.py``.

Same classes, constructor / ``forward`` / ``sample`` signatures, attributes and ``state_dict`` keys as the
reference (sda/score.py:15-396), so ``experiments/{lorenz,kolmogorov}`` run with ``import sda_amd as sda``.
What differs is where the arithmetic happens: the score evaluation (U-Net, window unfold/fold), the
predictor-corrector updates and the guidance glue run as hand-written gfx950 kernels (libsda_hip.so);
torch is used for device memory, the RNG streams (same calls in the same order as the reference) and for
differentiating a user-supplied observation operator ``A``.  No CPU path exists: CPU tensors raise.
"""

import math
import threading
from typing import Callable, Optional, Union

import torch
import torch.nn as nn
from torch import Size, Tensor
from tqdm import tqdm

from . import ops
from . import training
from ._lib import SdaHipError
from .engine import Source, attach_context, run_unet, source_from_tensor
from .nn import *  # noqa: F401,F403  (the reference re-exports its nn module the same way, score.py:12)
from .nn import ResMLP, UNet


def broadcast(*tensors: Tensor, ignore: Union[int, list] = 0):
    r"""Broadcasts tensors together except their last ``ignore`` dims (zuko.utils.broadcast; shape-only)."""
    if type(ignore) is int:
        ignore = [ignore] * len(tensors)
    split = [t.dim() - i for t, i in zip(tensors, ignore)]
    common = torch.broadcast_shapes(*(t.shape[:s] for t, s in zip(tensors, split)))
    return [torch.broadcast_to(t, common + t.shape[s:]) for t, s in zip(tensors, split)]


class TimeEmbedding(nn.Sequential):
    r"""[cos(pi j t), sin(pi j t)]_{j=1..16} -> Linear(32,256) -> SiLU -> Linear(256, features)  (score.py:15-35)."""

    def __init__(self, features: int):
        super().__init__(nn.Linear(32, 256), nn.SiLU(), nn.Linear(256, features))
        self.register_buffer('freqs', torch.pi * torch.arange(1, 16 + 1))

    def forward(self, t: Tensor) -> Tensor:
        ops._dev(t)
        shape = t.shape
        if training.active(self):
            # training route: (T x 32) x (32 x 256) and (T x 256) x (256 x E) GEMMs under torch autograd, so that the gradient
            # of the modulation rows reaches these Linears (a sliver of a training step; the sampling path keeps the kernel)
            ang = t.reshape(-1, 1) * self.freqs
            h = torch.nn.functional.silu(self[0](torch.cat((torch.cos(ang), torch.sin(ang)), dim=-1)))
            return self[2](h).reshape(*shape, -1)
        emb = ops.time_embed(t.reshape(-1).contiguous(), self.freqs, self[0].weight.detach(), self[0].bias.detach(),
                             self[2].weight.detach(), self[2].bias.detach())
        return emb.reshape(*shape, -1)


class ScoreNet(nn.Module):
    r"""Score network on flat feature vectors: ResMLP over cat(x, emb(t)[, c])  (score.py:38-63)."""

    def __init__(self, features: int, context: int = 0, embedding: int = 16, **kwargs):
        super().__init__()
        self.embedding = TimeEmbedding(embedding)
        self.network = ResMLP(features + context + embedding, features, **kwargs)

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        emb = self.embedding(t)
        if c is None:
            x, emb = broadcast(x, emb, ignore=1)
            feats = torch.cat((x, emb), dim=-1)
        else:
            x, emb, c = broadcast(x, emb, c, ignore=1)
            feats = torch.cat((x, emb, c), dim=-1)
        return self.network(feats)


class _ForwardProbe(threading.local):
    """Armed while ``MCScoreNet`` asks a ``ScoreUNet`` subclass what its ``forward`` override hands on to ``ScoreUNet.forward``
    (see ``_context_only_override``): ``calls`` collects the argument tuples, ``out`` is the placeholder returned instead of
    running the network."""
    calls = None
    out = None


_probe = _ForwardProbe()


def _context_only_override(kernel: 'ScoreUNet', shape, t: Tensor, c: Optional[Tensor]):
    """Does ``kernel.forward(x, t, c)`` amount to ``ScoreUNet.forward(kernel, x, t, c')`` for some context ``c'``?

    That is the shape of the reference's own ``LocalScoreUNet`` (experiments/kolmogorov/utils.py:45-46: ``return
    super().forward(x, t, self.forcing)``), whose nets ``make_score`` builds when the reference's driver files run unchanged on
    this package.  The override is executed once on a storage-less placeholder of the unfolded shape with ``ScoreUNet.forward``
    recording its arguments instead of launching; if it was entered exactly once, with the placeholder and ``t`` untouched, and
    its result came back unchanged, the override only chose the context and ``(True, c')`` is returned -- the fused window
    path may then stand in for ``fold(kernel(unfold(x)))``.  Anything else (arithmetic on x, several calls, post-processing,
    an exception on the placeholder) answers ``(False, None)`` and the caller runs the override for real."""
    if type(kernel).forward is ScoreUNet.forward:
        return True, kernel._context(c)
    key = (type(kernel), tuple(shape))
    if key in _not_context_only:                 # (a refused override is not executed a second time per evaluation: its side effects fire once)
        return False, None
    ph = torch.empty(shape, device='meta')
    out = torch.empty(shape, device='meta')
    # in-place arithmetic keeps object identity (`x.mul_(0.5); return super().forward(x, t, c)`, `out = super()...; out.mul_(2)`):
    # the version counters of the placeholder, the result and t tell (meta tensors carry them)
    v_ph, v_out, v_t = ph._version, out._version, t._version if isinstance(t, Tensor) else None
    _probe.calls, _probe.out = [], out
    try:
        res = type(kernel).forward(kernel, ph, t, c)
        calls = _probe.calls
    except Exception:  # noqa: BLE001 -- an override that cannot digest the placeholder simply takes the generic path
        _not_context_only.add(key)
        return False, None
    finally:
        _probe.calls, _probe.out = None, None
    untouched = ph._version == v_ph and out._version == v_out and (v_t is None or t._version == v_t)
    if untouched and len(calls) == 1 and res is out and calls[0][0] is kernel and calls[0][1] is ph and calls[0][2] is t:
        return True, kernel._context(calls[0][3])
    _not_context_only.add(key)
    return False, None


_not_context_only = set()                        # (kernel class, unfolded shape) whose override was probed and refused


class ScoreUNet(nn.Module):
    r"""U-Net score network (score.py:66-93): context channels concatenated, batch dims flattened, t embedded."""

    def __init__(self, channels: int, context: int = 0, embedding: int = 64, **kwargs):
        super().__init__()
        self.embedding = TimeEmbedding(embedding)
        self.network = UNet(channels + context, channels, embedding, **kwargs)

    def _context(self, c: Optional[Tensor]) -> Optional[Tensor]:
        """Hook for subclasses that inject their own context (e.g. the Kolmogorov forcing channel)."""
        return c

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        if _probe.calls is not None:                     # (an MCScoreNet is asking what a subclass passes on; nothing runs)
            _probe.calls.append((self, x, t, c))
            return _probe.out
        c = self._context(c)
        ops._dev(x, t, c)
        spatial = self.network.spatial
        if spatial == 3:
            return self._forward3d(x, t, c)
        xv, src = source_from_tensor(x, spatial)
        attach_context(src, c, spatial)
        emb = self.embedding(t.reshape(-1))
        out = run_unet(self.network, src, emb, x)
        return out.reshape(x.shape)

    def _forward3d(self, x: Tensor, t: Tensor, c: Optional[Tensor]) -> Tensor:
        """``spatial=3`` (score.py:81-93 as written: context channels concatenated, batch axes flattened): the general 3-D
        engine takes one planar tensor, so the concat is materialised here."""
        from .engine3d import run_unet3d
        feats = x
        if c is not None:
            batch = torch.broadcast_shapes(x.shape[:-4], c.shape[:-4])
            feats = torch.cat((x.expand(batch + x.shape[-4:]), c.expand(batch + c.shape[-4:])), dim=-4)
        out = run_unet3d(self.network, feats.reshape((-1,) + tuple(feats.shape[-4:])), self.embedding(t.reshape(-1)))
        return out.reshape(x.shape)

    def grad_bytes_per_sample(self, x_shape) -> Optional[int]:
        """HBM the input-VJP keeps alive per row of a batch ``x_shape`` = (B, C, *spatial); None when ``x_shape`` has no
        single leading batch axis (see GaussianScore._groups)."""
        spatial = self.network.spatial
        if len(x_shape) != spatial + 2 or spatial == 3:
            return None
        sp = tuple(x_shape)[-spatial:]
        h, w = (1, sp[0]) if spatial == 1 else sp
        return self.network.engine().bytes_per_image(h, w, True)


class MCScoreWrapper(nn.Module):
    r"""Disguises a `ScoreUNet` as a score network for a Markov chain (score.py:96-110).

    The (B, L, C) <-> (B, C, L) transposes stay views: the first convolution reads the trajectory through its
    strides."""

    def __init__(self, score: nn.Module):
        super().__init__()
        self.score = score

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        return self.score(x.transpose(1, 2), t, c).transpose(1, 2)

    def grad_bytes_per_sample(self, x_shape) -> Optional[int]:
        f = getattr(self.score, 'grad_bytes_per_sample', None)
        if f is None or len(x_shape) != 3:
            return None
        return f((x_shape[0], x_shape[2], x_shape[1]))


class _MCScoreFunction(torch.autograd.Function):
    """fold(kernel(unfold(x))) for a U-Net kernel without materialising the unfolded tensor (score.py:134-164).

    Forward: the head convolution reads windows straight out of x through a two-level batch stride; the tail's output
    goes through the selective-gather ``fold`` kernel.  Backward: fold adjoint -> U-Net VJP -> overlapping-window
    unfold adjoint (the one place overlaps sum)."""

    @staticmethod
    def forward(ctx, x: Tensor, kernel: 'ScoreUNet', order: int, emb: Tensor, c: Optional[Tensor], mod_all: Optional[Tensor] = None,
                *params):
        # (training route, sda_amd.training: mod_all formed differentiably by the caller, params = the engine's train_params())
        unet = kernel.network
        engine = unet.engine()
        B, L, C = x.shape[0], x.shape[1], x.shape[2]
        H, W = (1, x.shape[3]) if unet.spatial == 1 else (x.shape[3], x.shape[4])
        hw = H * W
        nw = L - 2 * order
        wl = 2 * order + 1
        if nw < 1:
            raise SdaHipError(f'trajectory of length {L} is shorter than the window {wl}')
        src = Source(x=x, n=B * nw, cx=wl * C, hs=H, ws=W, sn_outer=L * C * hw, sn_inner=C * hw, n_inner=nw, sc=hw,
                     sy=W, sx=1)
        attach_context(src, c, unet.spatial)
        T = emb.shape[0]
        if T not in (1, src.n):
            raise SdaHipError(f'time embedding batch {T} does not broadcast against {src.n} windows')
        per_image = T != 1
        train = len(params) > 0
        if not train:
            mod_all = engine.modulation(emb) if engine.mod_total > 0 else None
        need = any(ctx.needs_input_grad)
        dev = x.device
        s = torch.empty(src.n, wl * C, H, W, device=dev, dtype=torch.float32)
        ctx.vjp_state = engine.forward_all(src, mod_all, per_image, s, need, train)
        ctx.params, ctx.n_in = params, 6 + len(params)
        out = torch.empty_like(x)
        ops.fold(s, B, nw, order, C, hw, out)
        ctx.engine, ctx.src, ctx.mod_all, ctx.per_image = engine, src, mod_all, per_image
        ctx.geom = (B, nw, order, C, H, W)
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        engine, src = ctx.engine, ctx.src
        B, nw, order, C, H, W = ctx.geom
        hw, wl = H * W, 2 * order + 1
        dev = g.device
        g = g.contiguous()
        g_s = torch.empty(src.n, wl * C, H, W, device=dev, dtype=torch.float32)
        ops.fold_adjoint(g, B, nw, order, C, hw, g_s)
        if ctx.params:
            return _MCScoreFunction._train_backward(ctx, g_s)
        g_win = torch.empty(src.n, wl * C, H, W, device=dev, dtype=torch.float32)
        engine.backward_all(ctx.vjp_state, g_s, src, ctx.mod_all, ctx.per_image, g_win)
        g_x = torch.empty(B, nw + 2 * order, C, H, W, device=dev, dtype=torch.float32)
        ops.unfold_adjoint(g_win, B, nw, order, C, hw, wl * C, g_x)
        return g_x.reshape(ctx.x_shape), None, None, None, None

    @staticmethod
    def _train_backward(ctx, g_s: Tensor):
        from .engine import ParamGrads
        engine, src = ctx.engine, ctx.src
        B, nw, order, C, H, W = ctx.geom
        hw, wl = H * W, 2 * order + 1
        need_x, need_mod, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[5], any(ctx.needs_input_grad[6:])
        g_win = torch.empty(src.n, wl * C, H, W, device=g_s.device, dtype=torch.float32) if need_x else None
        pg = ParamGrads(ctx.mod_all, ctx.per_image, need_mod) if (need_p or need_mod) else None
        engine.backward_all(ctx.vjp_state, g_s, src, ctx.mod_all, ctx.per_image, g_win, pg)
        ctx.vjp_state = None
        g_x = None
        if need_x:
            g_x = torch.empty(B, nw + 2 * order, C, H, W, device=g_s.device, dtype=torch.float32)
            ops.unfold_adjoint(g_win, B, nw, order, C, hw, wl * C, g_x)
            g_x = g_x.reshape(ctx.x_shape)
        grads = engine.param_grads(pg, list(ctx.params)) if need_p else [None] * len(ctx.params)
        return (g_x, None, None, None, None, None if pg is None else pg.gmod, *grads)


class _FoldFunction(torch.autograd.Function):
    """``MCScoreNet.fold`` (score.py:155-164) as a HIP gather with its adjoint."""

    @staticmethod
    def forward(ctx, s: Tensor, order: int):
        s = s.contiguous()
        B, nw = s.shape[0], s.shape[1]
        wl = 2 * order + 1
        C = s.shape[2] // wl
        rest = s.shape[3:]
        hw = 1
        for r in rest:
            hw *= r
        out = torch.empty(B, nw + 2 * order, C, *rest, device=s.device, dtype=torch.float32)
        ops.fold(s, B, nw, order, C, hw, out)
        ctx.geom = (B, nw, order, C, hw, s.shape)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        B, nw, order, C, hw, shape = ctx.geom
        g_s = torch.empty(shape, device=g.device, dtype=torch.float32)
        ops.fold_adjoint(g.contiguous(), B, nw, order, C, hw, g_s)
        return g_s, None


class MCScoreNet(nn.Module):
    r"""Score network for a Markov chain: the score of a long trajectory composed from scores over windows of
    ``2*order+1`` frames (score.py:113-164).  ``kernel`` is reassignable, as the reference's drivers do."""

    def __init__(self, features: int, context: int = 0, order: int = 1, **kwargs):
        super().__init__()
        self.order = order
        build = ScoreUNet if kwargs.get('spatial', 0) > 0 else ScoreNet
        self.kernel = build(features * (2 * order + 1), context, **kwargs)

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        kernel = self.kernel
        fused = isinstance(kernel, ScoreUNet) and x.dim() == kernel.network.spatial + 3 \
            and kernel.network.spatial != 3 \
            and not (kernel._forward_hooks or kernel._forward_pre_hooks)         # (3-D kernels, hooked kernels: the generic path)
        ctx_c = None
        if fused:
            # a subclass whose forward only supplies the context (the reference's LocalScoreUNet) is as good as the stock one
            wl = 2 * self.order + 1
            fused, ctx_c = _context_only_override(
                kernel, (x.shape[0], max(x.shape[1] - 2 * self.order, 0), wl * x.shape[2]) + tuple(x.shape[3:]), t, c)
        if fused:
            ops._dev(x, t)
            ops._dev(ctx_c)
            emb = kernel.embedding(t.reshape(-1))
            xin = x if x.is_contiguous() else x.contiguous()
            if training.active(kernel.network):
                training.check_supported(kernel)
                engine = kernel.network.engine()
                mod_all = engine.modulation_train(emb) if engine.mod_total > 0 else None
                return _MCScoreFunction.apply(xin, kernel, self.order, emb, ctx_c, mod_all, *engine.train_params())
            return _MCScoreFunction.apply(xin, kernel, self.order, emb, ctx_c)
        # generic kernel (ScoreNet, or a user subclass overriding forward): unfold as a view + one gather copy
        s = kernel(self.unfold(x, self.order), t, c)
        return self.fold(s, self.order)

    def grad_bytes_per_sample(self, x_shape) -> Optional[int]:
        """HBM the input-VJP keeps alive per trajectory of a batch ``x_shape`` = (B, L, C, *spatial): one U-Net image per
        window.  None for kernels that are not U-Nets (small activations) and for unbatched trajectories."""
        if not isinstance(self.kernel, ScoreUNet) or len(x_shape) != self.kernel.network.spatial + 3:
            return None
        per = self.kernel.grad_bytes_per_sample((1,) + tuple(x_shape)[2:])
        return None if per is None else max(x_shape[1] - 2 * self.order, 1) * per

    @staticmethod
    def unfold(x: Tensor, order: int) -> Tensor:
        r"""(B, L, C, ...) -> (B, L-2k, (2k+1)C, ...)."""
        x = x.unfold(1, 2 * order + 1, 1)
        x = x.movedim(-1, 2)
        return x.flatten(2, 3)

    @staticmethod
    def fold(x: Tensor, order: int) -> Tensor:
        r"""Selective gather back to (B, L, C, ...): first window's leading slots, every centre, last window's
        trailing slots.  Not an overlap-add."""
        ops._dev(x)
        return _FoldFunction.apply(x, order)


class VPSDE(nn.Module):
    r"""Noise scheduler for the variance preserving SDE, :math:`\mu = \alpha`, :math:`\sigma^2 = 1-\alpha^2+\eta^2`,
    and the predictor-corrector sampler (score.py:167-276)."""

    def __init__(self, eps: nn.Module, shape: Size, alpha: str = 'cos', eta: float = 1e-3):
        super().__init__()
        self.eps = eps
        self.shape = shape
        self.dims = tuple(range(-len(shape), 0))
        self.eta = eta
        self.alpha_kind = alpha
        if alpha == 'lin':
            self.alpha = lambda t: 1 - (1 - eta) * t
        elif alpha == 'cos':
            self.alpha = lambda t: torch.cos(math.acos(math.sqrt(eta)) * t) ** 2
        elif alpha == 'exp':
            self.alpha = lambda t: torch.exp(math.log(eta) * t**2)
        else:
            raise ValueError()
        # the stock schedule lambda: mu_sigma() takes the fused-kernel path only while `alpha` is still this object
        object.__setattr__(self, '_alpha_stock', self.alpha)
        self.register_buffer('device', torch.empty(()))

    def mu(self, t: Tensor) -> Tensor:
        return self.alpha(t)

    def sigma(self, t: Tensor) -> Tensor:
        return (1 - self.alpha(t) ** 2 + self.eta ** 2).sqrt()

    def mu_sigma(self, t: Tensor):
        """(mu(t), sigma(t)).  For a device-resident scalar t and the stock schedules both come from one HIP launch (as
        adjacent elements of one buffer, which the elementwise kernels take as their device coefficient pair); anything
        else -- batched t, CPU tensors, subclasses overriding mu / sigma / alpha -- goes through mu() and sigma()."""
        cls = type(self)
        kind = _SIGMA_KINDS.get(cls.sigma)
        stock_alpha = self.alpha is self._alpha_stock and not any('alpha' in k.__dict__ for k in cls.__mro__)
        if (torch.is_tensor(t) and t.is_cuda and t.numel() == 1 and t.dtype == torch.float32 and kind is not None
                and cls.mu is VPSDE.mu and stock_alpha and self.alpha_kind in _ALPHA_KINDS):
            ak = _ALPHA_KINDS[self.alpha_kind]
            k = (0.0, math.acos(math.sqrt(self.eta)), math.log(self.eta))[ak]
            pair = ops.vp_schedule(t.reshape(1), ak, self.eta, k, kind)
            return pair[0].reshape(t.shape), pair[1].reshape(t.shape)
        return self.mu(t), self.sigma(t)

    def forward(self, x: Tensor, t: Tensor, train: bool = False) -> Tensor:
        r"""Samples from the perturbation kernel p(x(t) | x)."""
        t = t.reshape(t.shape + (1,) * len(self.shape))
        eps = torch.randn_like(x)
        x = self.mu(t) * x + self.sigma(t) * eps
        return (x, eps) if train else x

    #: optional ``callable(step, correction) -> Tensor`` replacing ``randn_like`` for the corrector noise, and an
    #: optional initial draw; both exist so that parity tests can inject the reference's CPU noise (RNG).
    noise_source: Optional[Callable[[int, int], Tensor]] = None
    initial_noise: Optional[Tensor] = None
    #: replay each diffusion step from a captured hipGraph (see PCSampler.capture); off by default
    use_graph: bool = False
    #: optional ``training.KeyedLossNoise``: ``loss()`` then draws t and eps keyed on (seed, row, training step) in one launch and reduces
    #: the squared error in two (csrc/train_loss.hip) instead of using torch's generator -- replayable from a hipGraph; None: the torch route
    loss_noise: Optional['training.KeyedLossNoise'] = None

    def sampler(self, shape: Size = (), c: Tensor = None, steps: int = 64, corrections: int = 0,
                tau: float = 1.0) -> 'PCSampler':
        r"""The predictor-corrector loop of :meth:`sample` as a steppable object (``sampler.step()`` advances one
        diffusion step in place; used by ``sample`` itself, by bench.py and by the multi-GPU driver)."""
        return PCSampler(self, tuple(shape), c, steps, corrections, tau)

    def sample(self, shape: Size = (), c: Tensor = None, steps: int = 64, corrections: int = 0,
               tau: float = 1.0) -> Tensor:
        r"""Samples from p(x(0)) with ``steps`` predictor steps and ``corrections`` Langevin corrections each."""
        sampler = self.sampler(shape, c, steps, corrections, tau)
        if self.use_graph and (self.noise_source is None or getattr(self.noise_source, 'graph_safe', False)):
            sampler.capture()
        for _ in tqdm(range(steps), ncols=88):
            sampler.step()
        return sampler.result()

    def loss(self, x: Tensor, c: Tensor = None, w: Tensor = None) -> Tensor:
        r"""The denoising loss (score.py:265-276), as a VALUE: what the reference's validation pass computes under ``no_grad``
        (sda/utils.py ``loop``).  The networks here form input gradients only, so a call that would need parameter gradients
        (grad mode on, trainable parameters) raises instead of returning a loss whose ``backward()`` trains nothing -- unless
        parameter gradients are switched on (``sda_amd.training``) and the network is one they are formed for."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.eps.parameters()):
            if training.enabled():
                training.check_supported(self.eps)
            else:
                raise NotImplementedError('training is outside the sampling hot path: parameter gradients are never formed. '
                                          'Evaluate the loss under torch.no_grad() (validation), or freeze the parameters, or '
                                          'switch parameter gradients on (sda_amd.training.parameter_gradients())')
        if self.loss_noise is not None:
            return self._keyed_loss(x, c, w)
        t = torch.rand(x.shape[0], dtype=x.dtype, device=x.device)
        x, eps = self.forward(x, t, train=True)
        err = (self.eps(x, t, c) - eps).square()
        if w is None:
            return err.mean()
        return (err * w).mean() / w.mean()


    def _keyed_loss(self, x: Tensor, c: Tensor = None, w: Tensor = None) -> Tensor:
        """The same loss with ``loss_noise``'s keyed draws: sda_loss_perturb, the network, sda_loss_mse (with its cotangent for backward).
        Advances neither torch's generator nor the step counter."""
        from . import fused1d
        noise = self.loss_noise
        sched = fused1d.stock_schedule(self)
        if sched is None:
            raise NotImplementedError('the keyed denoising loss serves the stock schedules (alpha lin / cos / exp of VPSDE, SubVPSDE, '
                                      'SubSubVPSDE); a subclass overriding mu / sigma / alpha takes loss_noise = None')
        ak, eta, k, kind = sched
        t, eps, xt = ops.loss_perturb(x, noise.seed, noise.row0, ak, eta, k, kind, step_dev=noise.counter(x.device))
        out = self.eps(xt, t, c)
        if w is not None:
            err = (out - eps).square()
            return (err * w).mean() / w.mean()
        return _KeyedMSE.apply(out.contiguous(), eps)


class _KeyedMSE(torch.autograd.Function):
    """mean((out - eps)^2) on sda_loss_mse; the cotangent g = (2 / numel)(out - eps) is formed in the forward's launch."""

    @staticmethod
    def forward(ctx, out, eps):
        loss, g = ops.loss_mse(out, eps, with_g=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        return g * grad_output, None


class PCSampler:
    r"""State of one ``VPSDE.sample`` call (score.py:225-263): x, the host-evaluated schedule and scratch buffers.

    The schedule is evaluated once on the host in fp32 with the reference's own formulas -- ``r = mu(t-dt)/mu(t)``,
    ``c1 = sigma(t-dt) - r sigma(t)`` (score.py:252-253) -- so no 0-dim device arithmetic or host sync happens per
    step; the updates themselves are in-place HIP kernels.

    ``capture()`` records one whole diffusion step (predictor + corrections, every score evaluation with its guidance
    VJP, RNG draws included) into a hipGraph and ``step()`` then replays it: the per-step scalars live in a device
    table indexed by a device-side step counter, so the replayed graph is step-independent.  This removes the Python /
    launch overhead that bounds the 1-D (Lorenz) configurations."""

    ROW = 5   # t, t - dt, r, c1, sigma(t - dt)

    def __init__(self, sde: VPSDE, shape, c, steps: int, corrections: int, tau: float):
        self.sde, self.shape, self.c = sde, shape, c
        self.steps, self.corrections, self.tau = steps, corrections, tau
        if sde.initial_noise is not None:
            x = sde.initial_noise.to(sde.device).clone()
        else:
            x = torch.randn(shape + tuple(sde.shape)).to(sde.device)       # host RNG then H2D, as the reference
        self.x = x.reshape(-1, *sde.shape).contiguous()
        ops._dev(self.x)
        self.nb = self.x.shape[0]
        time_cpu = torch.linspace(1, 0, steps + 1)
        self.dt = 1 / steps
        t_next = time_cpu[:-1] - self.dt
        mu_t, mu_n = sde.mu(time_cpu[:-1]), sde.mu(t_next)
        sg_t, sg_n = sde.sigma(time_cpu[:-1]), sde.sigma(t_next)
        r = mu_n / mu_t
        c1 = sg_n - r * sg_t
        self.r, self.c1, self.sg_n = r.tolist(), c1.tolist(), sg_n.tolist()
        self.time = time_cpu.to(sde.device)
        self._table_cpu = torch.stack((time_cpu[:-1], t_next, r, c1, sg_n), dim=1).contiguous()
        self.partial = torch.empty(self.nb * ops.SUMSQ_CHUNKS, device=self.x.device, dtype=torch.float32)
        self.i = 0
        self._graph = None
        # the six-launch step of sda_amd/fused1d.py when the job has the shape of experiments/lorenz/eval.py:72-84
        self._fused = None
        if c is None and type(sde.eps) is GaussianScore and self.x.dim() == 3:
            from . import fused1d
            self._fused = fused1d.plan(sde.eps, self.x, None, None)
            if self._fused is not None:
                self._table = self._table_cpu.to(self.x.device)
                self._istep = torch.zeros(1, device=self.x.device, dtype=torch.int64)

    # ------------------------------------------------------------------ eager step
    @torch.no_grad()
    def _eager_step(self, i: int):
        sde, x = self.sde, self.x
        t = self.time[i]
        # predictor: x <- r x + (sigma' - r sigma) eps(x, t)
        ops.pc_predict(x, sde.eps(x, t, self.c).contiguous(), self.r[i], self.c1[i])
        # corrector: Langevin steps with delta = tau / mean(eps^2)
        for j in range(self.corrections):
            z = torch.randn_like(x) if sde.noise_source is None else sde.noise_source(i, j).to(x)
            eps = sde.eps(x, t - self.dt, self.c).contiguous()
            nchunk = ops.sumsq_partial(eps, self.nb, self.partial)
            ops.pc_correct(x, eps, z.contiguous(), self.nb, self.partial, self.tau, self.sg_n[i], nchunk=nchunk)

    # ------------------------------------------------------------------ fused step (eager and captured alike)
    @torch.no_grad()
    def _fused_step(self, i: Optional[int]):
        """prologue, then per score evaluation two launches with the predictor update / the Langevin step-size sums in the second
        one's epilogue, then the corrector update: 3 + 3 C launches (general path: ~14 per evaluation + 7).  The step's scalars come
        from the device table row selected by the device step counter, which the prologue advances."""
        from .parallel import KeyedNoise
        sde, x, F = self.sde, self.x, self._fused
        F.prologue_step(self._table, self._istep)
        F.forward(x, 0)
        F.backward(1, 0, x=x)                                 # x <- r x + c1 eps(x, t)
        ns = sde.noise_source
        for j in range(self.corrections):
            F.forward(x, 1)
            F.backward(2, 1)                                  # eps(x, t - dt) and its per-tile sums of squares
            if type(ns) is KeyedNoise and tuple(ns.event) == tuple(x.shape[1:]) and ns.hi - ns.lo == self.nb \
                    and self.nb <= ops.PC_KEYED_MAX_ROWS:         # (the batch is grid.y there; larger: draw + general correction)
                ops.pc_correct_keyed(x, F.out, self.nb, F.partial, F.ptiles, self.tau, F.coef[6:7], ns.seed, ns.lo, F.step_i,
                                     ns.corrections, j)
            else:
                if ns is None:
                    z = torch.randn_like(x)
                elif i is None:
                    z = ns.draw_dev(F.step_i, j)
                else:
                    z = ns(i, j).to(x)
                ops.pc_correct(x, F.out, z.contiguous(), self.nb, F.partial, self.tau, 0.0, coef_dev=F.coef[6:7], nchunk=F.ptiles)

    # ------------------------------------------------------------------ graph-captured step
    @torch.no_grad()
    def _graph_body(self):
        if self._fused is not None:
            return self._fused_step(None)
        sde, x, cur = self.sde, self.x, self._cur
        cur.copy_(self._table.index_select(0, self._istep).reshape(-1))      # this step's scalars, device side
        ops.pc_predict(x, sde.eps(x, cur[0], self.c).contiguous(), 0.0, 0.0, coef_dev=cur[2:4])
        for j in range(self.corrections):
            z = torch.randn_like(x) if sde.noise_source is None else sde.noise_source.draw_dev(self._istep, j)
            eps = sde.eps(x, cur[1], self.c).contiguous()
            nchunk = ops.sumsq_partial(eps, self.nb, self.partial)
            ops.pc_correct(x, eps, z, self.nb, self.partial, self.tau, 0.0, coef_dev=cur[4:5], nchunk=nchunk)
        self._istep.add_(1)

    def capture(self):
        """Record one diffusion step into a hipGraph (torch.cuda.CUDAGraph).  Leaves x, the RNG streams and the step
        counter exactly as they were."""
        if self.sde.noise_source is not None and not getattr(self.sde.noise_source, 'graph_safe', False):
            raise SdaHipError('an injected noise_source cannot be captured into a graph (only device-keyed sources that '
                              'implement draw_dev, e.g. parallel.KeyedNoise, can)')
        dev = self.x.device
        if self._fused is None:
            self._table = self._table_cpu.to(dev)
            self._cur = torch.zeros(self.ROW, device=dev, dtype=torch.float32)
            self._istep = torch.full((1,), self.i, device=dev, dtype=torch.int64)
        keep_x = self.x.clone()
        keep_rng = torch.cuda.get_rng_state(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # warm-up off the capture stream (packs weights, sizes pools)
            self._graph_body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with ops.capture_without_gc(), torch.cuda.graph(graph):
            self._graph_body()
        self.x.copy_(keep_x)
        torch.cuda.set_rng_state(keep_rng, dev)
        self._istep.fill_(self.i)
        self._graph = graph
        return self

    def step(self):
        if self.i >= self.steps:
            raise StopIteration
        if self._graph is not None:
            self._graph.replay()
        elif self._fused is not None:
            self._fused_step(self.i)
        else:
            self._eager_step(self.i)
        self.i += 1

    def result(self) -> Tensor:
        return self.x.reshape(self.shape + tuple(self.sde.shape))


class SubVPSDE(VPSDE):
    r"""sub-VP SDE: :math:`\sigma = 1 - \alpha^2 + \eta` (score.py:279-288)."""

    def sigma(self, t: Tensor) -> Tensor:
        return 1 - self.alpha(t) ** 2 + self.eta


class SubSubVPSDE(VPSDE):
    r"""sub-sub-VP SDE: :math:`\sigma = 1 - \alpha + \eta` (score.py:291-302)."""

    def sigma(self, t: Tensor) -> Tensor:
        return 1 - self.alpha(t) + self.eta


_ALPHA_KINDS = {'lin': 0, 'cos': 1, 'exp': 2}
_SIGMA_KINDS = {VPSDE.sigma: 0, SubVPSDE.sigma: 1, SubSubVPSDE.sigma: 2}


def _mu_sigma(sde, t: Tensor):
    f = getattr(sde, 'mu_sigma', None)
    return f(t) if f is not None else (sde.mu(t), sde.sigma(t))


def _eps_with_vjp(sde: VPSDE, x: Tensor, t: Tensor, c, detach: bool):
    """eps = sde.eps(x) and a closure computing J_eps^T g (None when detached)."""
    if detach:
        with torch.no_grad():
            return sde.eps(x, t, c) if c is not None else sde.eps(x, t), None
    with torch.enable_grad(), training.input_only():     # (guidance: d/dx only, whatever the training switch says)
        xg = x.detach().requires_grad_(True)
        eps = sde.eps(xg, t, c) if c is not None else sde.eps(xg, t)

    def vjp(g: Tensor) -> Tensor:
        out, = torch.autograd.grad(eps, xg, g)
        return out
    return eps, vjp


def _linearizer(A):
    """``x -> (A(x), r -> J_A(x)^T r)`` for operators that bring their own VJP (sda_amd.observe: ``linearize``; any object with
    ``adjoint(r, x_shape)`` counts as linear), else None (torch autograd differentiates ``A``, as the reference does)."""
    lin = getattr(A, 'linearize', None)
    if lin is None and hasattr(A, 'adjoint'):
        return lambda xh: (A(xh), lambda r: A.adjoint(r, xh.shape))
    return lin


class DPSGaussianScore(nn.Module):
    r"""Diffusion posterior sampling guidance for p(y|x) = N(y | A(x), Sigma)  (score.py:305-344).
    Returns :math:`-\sigma(t) s(x(t), t | y)`.  Note ``err`` is summed over the whole batch, as in the reference."""

    #: set by ``parallel.sample_sharded`` for the duration of a sharded run: ``(lo, hi, batch, process_group)`` -- the rows
    #: of the global batch this rank holds.  ``err`` (score.py:339) is a sum over the WHOLE batch, the one real exchange
    #: step on the path: one scalar all-reduce per evaluation keeps a sharded run equal to the single-process one.
    shard: Optional[tuple] = None

    def __init__(self, y: Tensor, A: Callable[[Tensor], Tensor], sde: VPSDE, zeta: float = 1.0):
        super().__init__()
        self.register_buffer('y', y)
        self.A = A
        self.sde = sde
        self.zeta = zeta

    def _observed(self, ax: Tensor) -> Tensor:
        """A per-sample observation (leading axis = the global batch) follows this rank's rows; a shared one broadcasts."""
        sh = self.shard
        if sh is not None and self.y.dim() == ax.dim() and self.y.shape[0] == sh[2] and ax.shape[0] == sh[1] - sh[0]:
            return self.y[sh[0]:sh[1]]
        return self.y

    def _batch_total(self, err: Tensor) -> Tensor:
        if self.shard is not None and self.shard[3] is not None:
            import torch.distributed as dist
            dist.all_reduce(err, op=dist.ReduceOp.SUM, group=self.shard[3])
        return err

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        # (the reference's signature is (x, t); ``c`` is accepted and ignored so that VPSDE.sample, which always
        # passes it, can drive this module)
        mu, sigma = _mu_sigma(self.sde, t)
        eps, vjp = _eps_with_vjp(self.sde, x, t, None, False)
        eps_d = eps.detach().contiguous()
        xhat = torch.empty_like(eps_d)
        ops.denoise(x.contiguous(), eps_d, mu, sigma, xhat)
        lin = _linearizer(self.A)
        if lin is not None:
            # d/dx_hat sum (y - A x_hat)^2 = -2 J_A^T (y - A x_hat): no autograd through an operator with a hand-written VJP
            ax, a_vjp = lin(xhat)
            res = self._observed(ax) - ax
            err = self._batch_total(res.square().sum())
            cot = res * -2.0
            if cot.shape != ax.shape:
                cot = cot.sum_to_size(ax.shape)
            ghat = a_vjp(cot.contiguous())
        else:
            with torch.enable_grad():
                xhat.requires_grad_(True)
                ax = self.A(xhat)
                err = (self._observed(ax) - ax).square().sum()
            ghat, = torch.autograd.grad(err, xhat)
            err = self._batch_total(err.detach().clone())
        ghat = (ghat * (-self.zeta / err.detach().sqrt())).contiguous()      # d/dxhat of the DPS potential
        out = torch.empty_like(eps_d)
        ops.guided_combine(eps_d, ghat, vjp(ghat).contiguous(), mu, sigma, out)
        return out


def _reprime_scalars(module, incompatible_keys) -> None:
    module._prime_scalars()


class GaussianScore(nn.Module):
    r"""Likelihood guidance for Gaussian inverse problems, p(y|x) = N(y | A(x), std^2 + gamma (sigma/mu)^2)
    (score.py:347-396).  Returns :math:`-\sigma(t) s(x(t), t | y)`.

    ``x_hat = (x - sigma eps)/mu`` and the final combination are HIP kernels; ``A`` (an arbitrary callable) is
    differentiated by torch at ``x_hat``, and the chain rule back to ``x`` goes through the hand-written U-Net VJP:
    ``s = g/mu - (sigma/mu) J_eps^T g`` with ``g = d log p / d x_hat``."""

    def __init__(self, y: Tensor, A: Callable[[Tensor], Tensor], std: Union[float, Tensor], sde: VPSDE,
                 gamma: Union[float, Tensor] = 1e-2, detach: bool = False):
        super().__init__()
        self.register_buffer('y', y)
        self.register_buffer('std', torch.as_tensor(std))
        self.register_buffer('gamma', torch.as_tensor(gamma))
        self.A = A
        self.sde = sde
        self.detach = detach
        self._scalar_cache = None
        self._prime_scalars()
        self.register_load_state_dict_post_hook(_reprime_scalars)        # (a module-level function: the module stays picklable)

    def _prime_scalars(self):
        """Read std / gamma back NOW (construction, .to(), load_state_dict) so that the first guided evaluation -- possibly inside a
        hipGraph capture, where a device read-back is illegal -- finds the cache filled."""
        self._scalar_cache = None
        try:
            self._scalars
        except Exception:  # noqa: BLE001 -- e.g. meta tensors; the lazy path reports a real problem at first use
            self._scalar_cache = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._prime_scalars()
        return out

    @property
    def _scalars(self):
        """(std, gamma) as python floats when both buffers are scalars (every experiment of the reference): the likelihood
        cotangent is then one fused launch.  Read from the LIVE buffers -- ``load_state_dict``, ``gs.std = ...`` and in-place
        writes all change what the fused paths use, as they do for the general path -- and cached on the buffers' identity and
        version counter, so that a sampling loop pays the device read-back once (and none inside a graph capture)."""
        std, gamma = self.std, self.gamma
        if std.numel() != 1 or gamma.numel() != 1:
            return None
        ver = ops.tensor_version
        key = (std.data_ptr(), ver(std), std.device, gamma.data_ptr(), ver(gamma), gamma.device)
        hit = self._scalar_cache
        if hit is None or hit[0] != key:
            if std.is_cuda and torch.cuda.is_current_stream_capturing():
                raise SdaHipError('GaussianScore.std / gamma changed (fill_ / copy_ / a new tensor) and are first read inside a hipGraph '
                                  'capture, where the device read-back is illegal: evaluate the score once (or call '
                                  '_prime_scalars()) before capturing')
            hit = (key, (float(std), float(gamma)))
            self._scalar_cache = hit
        return hit[1]

    #: samples per streamed group: None = decide from free HBM, 0 = never split, n = force groups of n (tests)
    group_size: Optional[int] = None

    def _groups(self, x: Tensor, t: Tensor, c) -> Optional[int]:
        """log p(y|x) is a sum over samples and the variance is not learned, so the guidance gradient of one sample never
        depends on another: when the activations of the whole batch do not fit in HBM, the batch is streamed in groups
        of whole samples (forward -> likelihood -> VJP per group, nothing recomputed) instead of running every forward
        first and recomputing most of them in the backward."""
        if self.group_size == 0 or self.detach or c is not None or x.dim() < 2 or x.shape[0] < 2:
            return None
        if torch.is_tensor(t) and t.numel() > 1:
            return None
        B = x.shape[0]
        per = None
        for m in self.sde.eps.modules():                 # outermost network that knows its activation footprint
            f = getattr(m, 'grad_bytes_per_sample', None)
            if f is not None:
                per = f(tuple(x.shape))                  # None: x has no leading batch axis for this network
                break
        if not per:
            return None
        if self.group_size:
            return self.group_size if self.group_size < B else None
        if not x.is_cuda:
            return None
        from .engine import KEEP_HBM_FRACTION
        total = torch.cuda.get_device_properties(x.device).total_memory
        avail = max(total - torch.cuda.memory_allocated(x.device), total // 8)
        budget = 0.9 * KEEP_HBM_FRACTION * avail
        if per * B <= budget or per > budget:
            return None                                  # everything fits / not even one sample does (engine recomputes)
        ngroups = -(-B // int(budget // per))
        return -(-B // ngroups)

    def forward(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        return self._run(x, t, c, False)

    def log_p_grad(self, x: Tensor, t: Tensor, c: Tensor = None) -> Tensor:
        r""":math:`\nabla_x \log p(y | x)` alone -- the ``s`` of score.py:394 -- through the same kernels as :meth:`forward`
        (which returns ``eps - sigma s``); lets parity tests compare the guidance gradient without the cancellation of
        ``(eps - forward) / sigma``."""
        return self._run(x, t, c, True)

    def _run(self, x: Tensor, t: Tensor, c, grad_only: bool) -> Tensor:
        g = self._groups(x, t, c)
        if g is None:
            return self._guided(x, t, c, None, None, grad_only)
        x = x.contiguous()
        out = torch.empty_like(x, dtype=torch.float32)
        B = x.shape[0]
        for lo in range(0, B, g):
            hi = min(B, lo + g)
            self._guided(x[lo:hi], t, c, (lo, hi, B), out[lo:hi], grad_only)
        return out

    def _guided(self, x: Tensor, t: Tensor, c, rows, out: Tensor = None, grad_only: bool = False) -> Tensor:
        if rows is None and out is None and not grad_only:
            # the Lorenz shape of the reference's eval.py (1-D single-level U-Net, strided observation): two fused launches
            from . import fused1d
            fz = fused1d.plan(self, x, t, c)
            if fz is not None:
                return fz.evaluate(x, t)
        mu, sigma = _mu_sigma(self.sde, t)
        eps, vjp = _eps_with_vjp(self.sde, x, t, c, self.detach)
        eps_d = eps.detach().contiguous()

        ghat = None
        fused = getattr(self.A, 'gaussian_guidance', None)
        sc = self._scalars
        if fused is not None and sc is not None:
            # subsampling observation, scalar std / gamma: denoise + A + cotangent + A^T in one launch
            yq = self.y
            if rows is not None and yq.dim() == x.dim() and yq.shape[0] == rows[2]:
                yq = yq[rows[0]:rows[1]]
            ghat = fused(x.contiguous(), eps_d, yq, sc[0], sc[1], mu, sigma)
        if ghat is not None:
            return self._finish(eps_d, ghat, vjp, mu, sigma, out, grad_only)
        xhat = torch.empty_like(eps_d)
        ops.denoise(x.contiguous(), eps_d, mu, sigma, xhat)

        def observed(ax: Tensor) -> Tensor:
            # a per-sample observation follows its rows; a shared one broadcasts as in the reference
            if rows is not None and self.y.dim() == ax.dim() and self.y.shape[0] == rows[2]:
                return self.y[rows[0]:rows[1]]
            return self.y

        lin = _linearizer(self.A)
        if lin is not None:
            # operator with a hand-written (linearised) adjoint (sda_amd.observe): d log p / d x_hat = J_A(x_hat)^T((y - A x_hat)/var)
            # -- exactly what autograd.grad(log_p, x) propagates through A at sda/score.py:389-394, without building a graph
            ax, a_vjp = lin(xhat)
            yo = observed(ax)
            if (sc is not None and ax.dtype == torch.float32 and yo.dtype == torch.float32 and
                    (yo.shape == ax.shape or yo.shape == ax.shape[1:] or
                     (yo.dim() == ax.dim() and yo.shape[0] == 1 and yo.shape[1:] == ax.shape[1:]))):
                # (the same path for every batch size: sharded and single-rank runs take the same guidance kernels)
                cot = ops.gauss_cotangent(yo, ax, sc[0], sc[1], mu, sigma)
            else:
                var = self.std ** 2 + self.gamma * (sigma / mu) ** 2
                cot = ((yo - ax) / var).contiguous()
            if cot.shape != ax.shape:
                cot = cot.sum_to_size(ax.shape)
            ghat = a_vjp(cot.contiguous()).contiguous()
        else:
            with torch.enable_grad():
                xhat.requires_grad_(True)
                ax = self.A(xhat)
            # d/dx_hat of log p = -sum(err^2 / var) / 2 is A's VJP with cotangent err / var: autograd only has to go
            # through A itself, not through the scalar reduction (same value, a third of the launches)
            err = observed(ax) - ax.detach()
            var = self.std ** 2 + self.gamma * (sigma / mu) ** 2
            cot = err / var
            if cot.shape != ax.shape:
                cot = cot.sum_to_size(ax.shape)
            ghat, = torch.autograd.grad(ax, xhat, cot)
            ghat = ghat.contiguous()
        return self._finish(eps_d, ghat, vjp, mu, sigma, out, grad_only)

    def _finish(self, eps_d: Tensor, ghat: Tensor, vjp, mu, sigma, out, grad_only: bool) -> Tensor:
        if out is None:
            out = torch.empty_like(eps_d)
        v = None if vjp is None else vjp(ghat).contiguous()
        if grad_only:
            # combine(0, ghat, vjp) = -(sigma/mu)(ghat - sigma vjp) = -sigma s
            ops.guided_combine(torch.zeros_like(eps_d), ghat, v, mu, sigma, out)
            return out.div_(-torch.as_tensor(sigma, device=out.device))
        ops.guided_combine(eps_d, ghat, v, mu, sigma, out)
        return out
