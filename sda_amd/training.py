r"""Opt-in parameter gradients for the score U-Net (training).

By default this package forms input gradients only (the sampling hot path): ``VPSDE.loss`` refuses to run where it would have
to train, and a U-Net evaluated under grad mode with trainable parameters warns that their gradients are not formed.  With the
switch on, the U-Net's backward also forms the gradients of every convolution weight and bias (csrc/conv_wgrad.hip), of the
modulation rows and, through torch autograd on the small ``project`` / time-embedding GEMMs, of those Linears::

    import sda_amd
    with sda_amd.training.parameter_gradients():
        loss = sde.loss(x)
        loss.backward()
        optimizer.step()

Served: ``ScoreUNet`` (and subclasses such as the reference's ``LocalScoreUNet``) with ``spatial`` 1 or 2, alone, inside
``MCScoreNet`` or wrapped by ``MCScoreWrapper``, with the default fp32 multiply.  Anything else raises ``NotImplementedError``.

A second opt-in, ``parameter_gradients(mlp=True)`` (or ``enable(mlp=True)``), also serves ``ScoreNet`` -- a ``TimeEmbedding`` and a
``ResMLP`` --, alone or as the kernel of ``MCScoreNet`` through its generic route (unfold gather, ``ScoreNet`` on the window rows,
fold): the Lorenz local net of the reference's ``train_local``.  The ResMLP's backward is then three launches whatever its depth
(csrc/mlp_train.hip: the input VJP that also stores the cotangent of every GEMM's output, one weight-gradient launch for all
layers, one slab reduction; sda_amd/mlp.py), the time embedding trains through torch autograd as it does for the U-Nets.  The
``ResMLP`` must be one the whole-MLP kernels take (widths <= 256, biases, one activation, one LayerNorm eps); the fused window
kernels of the samplers stay sampling-only.  ``sda_amd.utils.loop`` switches both on.

A third opt-in, ``parameter_gradients(wgrad='tiled')`` (or ``enable(wgrad='tiled')``), sends the weight gradients of the 3 x 3,
stride-1 block convolutions (36 of the 42 launches of a Kolmogorov step) to the tiled kernel csrc/conv_wgrad3.hip; heads, tails, 1-D
nets and anything else outside its served set stay on the general kernel.  ``wgrad='tiled_ht'`` (heads and tails) is that route and,
beside it, the same kernel's two other geometries (sda_conv_wgrad3x) for the 3 x 3 stride-2 heads and the up-sampling tails with channel counts in multiples of 32 (4 more
of the 42 launches); the first head (context plane) and the last tail stay on the general kernel.  The default ``'general'`` is bitwise
what it always was, and so is ``'tiled'``.

A fourth opt-in, ``parameter_gradients(net1d=True)`` (or ``enable(net1d=True)``), trains a single-level 1-D U-Net the whole-net kernel
serves (csrc/net1d.hip: <= 64 channels, one padding mode, no context -- the Lorenz global net of the reference's ``train_global``) on
csrc/net1d_train.hip: one forward launch, three backward launches (the input VJP that also stores every convolution's output cotangent,
one weight-gradient launch for all convolutions, one slab reduction) and one pack launch after each parameter update.  Nets that
kernel declines, and a batch whose activations do not fit the memory budget in one piece, keep the per-layer route; the default
``False`` leaves every route bit for bit what it is.

:class:`AdamW` is the optimizer step of this route as one launch (csrc/optim.hip) that keeps the ResMLP weight slabs packed."""
import contextlib
import math
import threading
from ctypes import c_int32, c_int64

import torch

SUPPORTED = ('ScoreUNet (and subclasses such as LocalScoreUNet) with spatial = 1 or 2, alone, in MCScoreNet or in MCScoreWrapper, '
             "with the fp32 multiply (ops.MULTIPLY == 'f32')")

SUPPORTED_MLP = ('ScoreNet (TimeEmbedding + ResMLP of Linear layers and LayerNorm residual blocks: widths <= 256, biases present, one '
                 'activation, one LayerNorm eps), alone or as the kernel of MCScoreNet, on the device, '
                 "with the fp32 multiply (ops.MULTIPLY == 'f32'), under parameter_gradients(mlp=True)")

WGRAD_ROUTES = ('general', 'tiled', 'tiled_ht')

_enabled = False
_mlp = False
_wgrad = 'general'
_net1d = False
_local = threading.local()


def _check_route(wgrad: str) -> str:
    if wgrad not in WGRAD_ROUTES:
        raise ValueError(f"wgrad route {wgrad!r} (expected 'general', 'tiled' or 'tiled_ht')")
    return wgrad


def enable(mlp: bool = False, wgrad: str = 'general', net1d: bool = False) -> None:
    """Form parameter gradients in the U-Net backward from now on; ``mlp=True``: in the ScoreNet / ResMLP backward as well.
    ``wgrad='tiled'``: the 3 x 3 block convolutions' weight gradients on the tiled kernel (csrc/conv_wgrad3.hip) where it serves the
    launch; ``wgrad='tiled_ht'``: also the stride-2 heads and up-sampling tails on its two other geometries (sda_conv_wgrad3x); every other layer,
    and everything under the default ``'general'``, on the general kernel.  ``net1d=True``: single-level 1-D U-Nets the whole-net
    kernel serves train on csrc/net1d_train.hip."""
    global _enabled, _mlp, _wgrad, _net1d
    route = _check_route(wgrad)
    _enabled, _mlp, _wgrad, _net1d = True, bool(mlp), route, bool(net1d)


def disable() -> None:
    """Back to the default: input gradients only (and the general weight-gradient route)."""
    global _enabled, _mlp, _wgrad, _net1d
    _enabled, _mlp, _wgrad, _net1d = False, False, 'general', False


def enabled() -> bool:
    return _enabled


def mlp_enabled() -> bool:
    """Are parameter gradients of ScoreNet / ResMLP switched on (the second opt-in)?"""
    return _enabled and _mlp


def wgrad_route() -> str:
    """The weight-gradient route of the convolutions: 'general' (default), 'tiled' or 'tiled_ht' (the third opt-in)."""
    return _wgrad


def net1d_enabled() -> bool:
    """Do single-level 1-D U-Nets train on the whole-net kernels (the fourth opt-in)?"""
    return _enabled and _net1d


@contextlib.contextmanager
def parameter_gradients(on: bool = True, mlp: bool = False, wgrad: str = 'general', net1d: bool = False):
    """Switch parameter gradients on (or off) inside the block, those of ScoreNet / ResMLP with ``mlp=True``, the block convolutions'
    weight gradients on the tiled kernel with ``wgrad='tiled'``, the heads' and tails' as well with ``wgrad='tiled_ht'``, single-level
    1-D U-Nets on the whole-net kernels with ``net1d=True``; the previous state of all four switches is restored on exit."""
    global _enabled, _mlp, _wgrad, _net1d
    route = _check_route(wgrad)
    prev = (_enabled, _mlp, _wgrad, _net1d)
    _enabled, _mlp, _wgrad, _net1d = bool(on), bool(on) and bool(mlp), route, bool(on) and bool(net1d)
    try:
        yield
    finally:
        _enabled, _mlp, _wgrad, _net1d = prev


@contextlib.contextmanager
def input_only():
    """Inside the block a network evaluation forms input gradients only, whatever the switch says (the guidance VJPs of the
    samplers: their results stay bitwise those of the default route)."""
    depth = getattr(_local, 'input_only', 0)
    _local.input_only = depth + 1
    try:
        yield
    finally:
        _local.input_only = depth


def active(module: torch.nn.Module) -> bool:
    """Does an evaluation of ``module`` now take the parameter-gradient route?"""
    return (_enabled and torch.is_grad_enabled() and not getattr(_local, 'input_only', 0)
            and any(p.requires_grad for p in module.parameters()))


def mlp_active(module: torch.nn.Module) -> bool:
    """Does an evaluation of the ResMLP ``module`` now take the parameter-gradient route (csrc/mlp_train.hip)?"""
    return _mlp and active(module)


def served() -> str:
    """The served set as the refusals name it: the U-Nets, and with ``mlp=True`` ScoreNet."""
    return f'{SUPPORTED}; {SUPPORTED_MLP}' if mlp_enabled() else SUPPORTED


def check_mlp(network: torch.nn.Module) -> None:
    """Raise NotImplementedError unless ``network`` is a ResMLP the whole-MLP plan takes (the MLP training route runs nothing else)."""
    from . import mlp, ops
    if ops.MULTIPLY != 'f32':
        raise NotImplementedError(f'parameter gradients are formed with the fp32 multiply only (ops.MULTIPLY = {ops.MULTIPLY!r}); '
                                  f'supported: {served()}')
    layers = list(network)
    if not all(isinstance(l, torch.nn.Linear) or mlp._is_res_block(l) for l in layers) or mlp._fused_plan(layers) is None:
        raise NotImplementedError(f'parameter gradients of this {type(network).__name__} are not formed (the whole-MLP kernels do not take '
                                  f'it: a width above 256, a Linear without bias, mixed activations or eps, custom layers); '
                                  f'supported: {served()}')


def check_supported(net: torch.nn.Module) -> None:
    """Raise NotImplementedError unless every trainable parameter ``net`` reaches belongs to a served network: a U-Net, or with
    ``mlp=True`` a ScoreNet."""
    from . import ops
    from .nn import UNet
    from .score import ScoreNet, ScoreUNet
    if ops.MULTIPLY != 'f32':
        raise NotImplementedError(f'parameter gradients are formed with the fp32 multiply only (ops.MULTIPLY = {ops.MULTIPLY!r}); '
                                  f'supported: {served()}')
    covered = set()
    hint = ''
    for mod in net.modules():
        if isinstance(mod, ScoreNet):
            if mlp_enabled():
                check_mlp(mod.network)
                covered.update(id(p) for p in mod.parameters())
            else:
                hint = ' (a ScoreNet trains under parameter_gradients(mlp=True))'
        if isinstance(mod, (ScoreUNet, UNet)):
            spatial = mod.network.spatial if isinstance(mod, ScoreUNet) else mod.spatial
            if spatial not in (1, 2):
                raise NotImplementedError(f'parameter gradients of a spatial = {spatial} U-Net are not formed; '
                                          f'supported: {served()}')
            covered.update(id(p) for p in mod.parameters())
    for name, p in net.named_parameters():
        if p.requires_grad and id(p) not in covered:
            raise NotImplementedError(f'parameter {name!r} ({type(_owner(net, name)).__name__}) would receive no gradient: '
                                      f'supported: {served()}{hint}')


def _owner(net: torch.nn.Module, name: str) -> torch.nn.Module:
    mod = net
    for part in name.split('.')[:-1]:
        mod = getattr(mod, part)
    return mod


class AdamW(torch.optim.Optimizer):
    r"""AdamW (decoupled weight decay) whose step is this project's kernel (csrc/optim.hip): one launch per 32 tensors instead of
    torch's several per step, in the operation order of torch's single-tensor AdamW.  State (``step`` a CPU float32 scalar,
    ``exp_avg``, ``exp_avg_sq``) and ``state_dict()`` are torch's: a checkpoint moves between the two in both directions, and
    ``LambdaLR``, ``zero_grad`` and param groups work unchanged.

    ``net`` names the module whose ResMLPs are to stay packed: for every Linear of a ResMLP the whole-MLP kernels take, the launch
    also writes the new weight to its place in the plan's forward and transposed slabs and the new bias to the padded bias row
    (sda_amd/mlp.py ``_FusedPlan``), so that no re-pack follows the update.  Parameters outside any plan (U-Net convolutions, the
    time embedding) and everything when ``net`` is None take the plain update.  Every updated parameter's version counter is bumped
    as an in-place torch update bumps it: the caches keyed on it (the convolution weights, the fused window kernels) see the change.

    fp32 contiguous device parameters only; ``amsgrad``, ``maximize``, ``capturable``, ``differentiable`` and a tensor ``lr`` are
    refused (ValueError)."""

    _REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, net=None, **options):
        unknown = set(options) - set(self._REFUSED)
        if unknown:
            raise TypeError(f'AdamW: unexpected arguments {sorted(unknown)}')
        if torch.is_tensor(lr):
            raise ValueError('sda_amd.training.AdamW: a tensor lr is not supported (pass a float)')
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'sda_amd.training.AdamW: invalid hyperparameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}')
        # (the keys of torch.optim.AdamW's groups, so that a state_dict loads there without defaults being guessed)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        defaults.update(options)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)
        self._mlps = []
        if net is not None:
            from .nn import ResMLP
            self._mlps = [m for m in net.modules() if isinstance(m, ResMLP)]
        self._plans, self._slots = (), {}

    @classmethod
    def _check_group(cls, group):
        for name in cls._REFUSED:
            if group.get(name):
                raise ValueError(f'sda_amd.training.AdamW: {name}=True is not supported')
        if torch.is_tensor(group['lr']):
            raise ValueError('sda_amd.training.AdamW: a tensor lr is not supported (pass a float)')

    def _plan_slots(self):
        """{id(parameter): (plan, GEMM index, pack kind)} over the ResMLPs of ``net`` the whole-MLP kernels take; rebuilt when a plan
        was replaced (its layer list changed)."""
        from . import mlp
        plans = []
        for m in self._mlps:
            layers = list(m)
            if all(isinstance(l, torch.nn.Linear) or mlp._is_res_block(l) for l in layers):
                plan = mlp._fused_plan(layers)
                if plan is not None:
                    plans.append(plan)
        if len(plans) != len(self._plans) or any(a is not b for a, b in zip(plans, self._plans)):
            slots = {}
            for plan in plans:
                for g, (*_r, lin) in enumerate(plan.gemms):
                    slots.setdefault(id(lin.weight), (plan, g, 1))
                    slots.setdefault(id(lin.bias), (plan, g, 2))
            self._plans, self._slots = tuple(plans), slots
        return self._slots

    def _init_state(self, p):
        if not (p.is_cuda and p.dtype == torch.float32):
            raise ValueError(f'sda_amd.training.AdamW updates fp32 device tensors (got a {p.device.type} {p.dtype} parameter)')
        if not p.is_contiguous():
            raise ValueError('sda_amd.training.AdamW: a parameter is not contiguous')
        state = self.state[p]
        state['step'] = torch.tensor(0.0, dtype=torch.float32)
        state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        slots = self._plan_slots() if self._mlps else {}
        for group in self.param_groups:
            self._check_group(group)
            buckets = {}                                     # (device, step count) -> [(parameter, gradient, state)]
            for p in group['params']:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state = self._init_state(p)
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                    raise ValueError('sda_amd.training.AdamW: gradients are dense fp32 tensors on the parameter\'s device')
                state['step'] += 1
                buckets.setdefault((p.device, float(state['step'])), []).append((p, g if g.is_contiguous() else g.contiguous(), state))
            for (device, t), items in buckets.items():
                self._launch(group, device, t, items, slots)
        return loss

    def _launch(self, group, device, t, items, slots):
        from . import _lib, ops
        lr, (beta1, beta2), n = float(group['lr']), group['betas'], _lib.ADAMW_MAXT
        plans = {}
        for p, _g, _s in items:
            slot = slots.get(id(p))
            if slot is not None:
                plans[id(slot[0])] = slot[0]
        for plan in plans.values():
            plan._pack()                                     # (a no-op when the key hits; re-allocates after, say, a load_state_dict)
        with torch.cuda.device(device):
            for i0 in range(0, len(items), n):
                part = items[i0:i0 + n]
                pad = [0] * (n - len(part))
                d = _lib.AdamWDesc()
                d.ntensor = len(part)
                d.decay, d.one_m_beta1, d.beta2, d.one_m_beta2 = 1.0 - lr * group['weight_decay'], 1.0 - beta1, beta2, 1.0 - beta2
                d.step_size, d.rsqrt_bc2, d.eps = lr / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t), group['eps']
                fwd, bwd, kind, out_f, in_f = [], [], [], [], []
                for p, _g, state in part:
                    if not p.is_contiguous():
                        raise ValueError('sda_amd.training.AdamW: a parameter is not contiguous')
                    slot = slots.get(id(p))
                    if slot is None:
                        fwd.append(0); bwd.append(0); kind.append(0); out_f.append(0); in_f.append(0)
                        continue
                    plan, g, k = slot
                    _kk, i, o, _lin = plan.gemms[g]
                    kind.append(k); out_f.append(o); in_f.append(i)
                    if k == 1:
                        fwd.append(plan.wf.data_ptr() + 4 * plan.w_off[g]); bwd.append(plan.wb.data_ptr() + 4 * plan.w_off[g])
                    else:
                        fwd.append(plan.bias.data_ptr() + 4 * plan.b_off[g]); bwd.append(0)
                ptrs = _lib.c_fp * n
                d.p = ptrs(*[p.data_ptr() for p, _g, _s in part], *pad)
                d.g = ptrs(*[g.data_ptr() for _p, g, _s in part], *pad)
                d.m = ptrs(*[s['exp_avg'].data_ptr() for _p, _g, s in part], *pad)
                d.v = ptrs(*[s['exp_avg_sq'].data_ptr() for _p, _g, s in part], *pad)
                d.fwd, d.bwd = ptrs(*fwd, *pad), ptrs(*bwd, *pad)
                d.numel = (c_int64 * n)(*[p.numel() for p, _g, _s in part], *pad)
                d.pack_kind, d.out_f, d.in_f = (c_int32 * n)(*kind, *pad), (c_int32 * n)(*out_f, *pad), (c_int32 * n)(*in_f, *pad)
                ops.adamw_step(d)
        # the parameters changed as under an in-place torch update: bump their version counters (no launch), then tell the plans that
        # their slabs already hold the new values
        torch.autograd.graph.increment_version([p for p, _g, _s in items])
        for plan in plans.values():
            plan._key = plan._pack_key()
