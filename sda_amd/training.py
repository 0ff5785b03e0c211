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

:class:`AdamW` is the optimizer step of this route as one launch (csrc/optim.hip) that keeps the ResMLP weight slabs packed.
:class:`GraphedStep` replays a whole step -- the keyed denoising loss of :class:`KeyedLossNoise` (csrc/train_loss.hip), backward, the
optimizer launches with their step scalars in a device table -- as one hipGraph; ``utils.loop(graph=True)`` drives it."""
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


def step_scalars(lr: float, betas, weight_decay: float, t: float):
    """(decay, step_size, rsqrt_bc2) of optimizer step ``t`` (1, 2, ...), formed in double: what ``AdamW`` passes by value to
    sda_adamw_step and what ``GraphedStep`` writes (rounded to fp32 in both) to the table sda_adamw_step_dev reads."""
    beta1, beta2 = betas
    return 1.0 - lr * weight_decay, lr / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t)


def scalar_rows(lr: float, betas, weight_decay: float, t0: float, rows: int) -> torch.Tensor:
    """The fp32 CPU table [rows][3] of ``step_scalars`` for the optimizer steps t0 + 1 ... t0 + rows (``GraphedStep``'s device table): each
    double is rounded to fp32 once, as the by-value descriptor fields round it."""
    return torch.tensor([step_scalars(lr, betas, weight_decay, t0 + 1 + r) for r in range(rows)], dtype=torch.float64).to(torch.float32)


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

    def _descriptors(self, group, items, slots):
        """The launches of ``items`` [(parameter, gradient, state)] as descriptors of up to 32 tensors, filled but for the three scalars of
        the step ({decay, step_size, rsqrt_bc2}: by value in ``_launch``, a device table row in ``GraphedStep``), and the plans whose slabs
        the pack epilogue writes (packed here: a no-op when their key hits; re-allocates after, say, a load_state_dict)."""
        from . import _lib
        (beta1, beta2), n = group['betas'], _lib.ADAMW_MAXT
        plans = {}
        for p, _g, _s in items:
            slot = slots.get(id(p))
            if slot is not None:
                plans[id(slot[0])] = slot[0]
        for plan in plans.values():
            plan._pack()
        descs = []
        for i0 in range(0, len(items), n):
            part = items[i0:i0 + n]
            pad = [0] * (n - len(part))
            d = _lib.AdamWDesc()
            d.ntensor = len(part)
            d.one_m_beta1, d.beta2, d.one_m_beta2, d.eps = 1.0 - beta1, beta2, 1.0 - beta2, group['eps']
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
            descs.append(d)
        return descs, plans

    def _launch(self, group, device, t, items, slots):
        from . import ops
        descs, plans = self._descriptors(group, items, slots)
        with torch.cuda.device(device):
            for d in descs:
                d.decay, d.step_size, d.rsqrt_bc2 = step_scalars(float(group['lr']), group['betas'], group['weight_decay'], t)
                ops.adamw_step(d)
        # the parameters changed as under an in-place torch update: bump their version counters (no launch), then tell the plans that
        # their slabs already hold the new values
        torch.autograd.graph.increment_version([p for p, _g, _s in items])
        for plan in plans.values():
            plan._key = plan._pack_key()


class KeyedLossNoise:
    """The draws of the denoising loss keyed on (seed, global row, training step) instead of torch's generator (csrc/train_loss.hip):
    in step ``s`` the noise of row ``b`` is row ``row0 + b`` of ``ops.randn_rows(seed, draw = 2 s)`` and its time a uniform from draw
    ``2 s + 1``.  ``s`` lives in a device int64 scalar (``counter``), so a captured training step replays; ``VPSDE.loss`` reads it and never
    advances it -- the caller (``step += 1``) or :class:`GraphedStep` does.  Set ``sde.loss_noise = KeyedLossNoise(seed)`` to take the route."""

    def __init__(self, seed: int, row0: int = 0, counter: torch.Tensor = None):
        if row0 < 0:
            raise ValueError('KeyedLossNoise: row0 >= 0')
        self.seed, self.row0 = int(seed), int(row0)
        self._counter, self._start = counter, 0

    def counter(self, device=None) -> torch.Tensor:
        """The device int64 scalar holding the step index (allocated on ``device`` at first use)."""
        if self._counter is None:
            self._counter = torch.full((1,), self._start, device=device if device is not None else 'cuda', dtype=torch.int64)
        return self._counter

    @property
    def step(self) -> int:
        """The step index (reading it waits for the device)."""
        return self._start if self._counter is None else int(self._counter.item())

    @step.setter
    def step(self, s: int) -> None:
        if s < 0:
            raise ValueError('KeyedLossNoise: step >= 0')
        if self._counter is None:
            self._start = int(s)
        else:
            self._counter.fill_(int(s))




class GraphedStep:
    r"""One training step -- keyed denoising loss, backward, AdamW -- replayed as ONE hipGraph.

        opt = sda_amd.training.AdamW(sde.parameters(), lr=1e-3, net=sde)
        stepper = sda_amd.training.GraphedStep(sde, opt, seed=0)
        loss = stepper.step(x)                # a 0-dim device tensor, valid until the next step

    The body of a step is ``sde.loss(x, c)`` under ``parameter_gradients(mlp, wgrad, net1d)`` with a :class:`KeyedLossNoise`, ``backward()``,
    the optimizer's launches in their replayable form (sda_adamw_step_dev: {decay, step_size, rsqrt_bc2} are a row of a device table of
    the next ``rows`` steps, selected by a device counter), ``loss_sum += loss`` and the increment of both device counters.  The first
    ``step`` runs that body uncaptured on a side stream (a real step) and then captures it for the batch's shape; later steps of that
    shape copy ``x`` into the static input and replay.  A batch of another shape (an epoch's short last batch) runs the body uncaptured:
    same kernels, same draws, same result.  The table is rebuilt, without a device synchronisation, when its rows run out or a group's
    ``lr`` or ``weight_decay`` changed (``LambdaLR``); a changed ``betas`` or ``eps`` (by value in the launches) captures again.

    A replay always computes with the current parameters: the packed weights the step reads are either written by the optimizer launch
    itself (the ResMLP slabs of ``AdamW(net=...)``; re-packed into place when a parameter was changed from outside) or re-packed by launches
    recorded at the head of the graph (everything else).  After every replay the parameters' version counters are bumped, so every cache
    outside the graph sees the update.  The optimizer's ``state[p]['step']`` counts are advanced lazily: before ``state_dict()``,
    ``load_state_dict()`` or a direct ``optimizer.step()`` observe them, or on request (``sync_state()``).

    Parameters, optimizer state and ``c`` keep their storage while a graph is alive (``optimizer.load_state_dict`` drops the graph: the
    next step captures again).  fp32 multiply only.

    ``GraphedStep(..., data=ds, batch_size=B)`` with a ``sda_amd.data.DeviceTrajectories`` feeds itself: ``step()`` takes no batch, the
    body begins with ``ds.draw(B, out=<the static input>)`` (one gather launch reading the dataset's device cursor, and its increment), so
    a replay copies nothing in.  An epoch's short last batch, known from the dataset's host mirror, runs the same body uncaptured on
    ``ds.draw(B)``.  Without ``data=`` nothing changes."""

    def __init__(self, sde, optimizer, *, seed: int, c: torch.Tensor = None, rows: int = 1024, mlp: bool = True, wgrad: str = 'general',
                 net1d: bool = False, data=None, batch_size: int = None):
        from . import ops
        if not isinstance(optimizer, AdamW):
            raise TypeError(f'GraphedStep drives sda_amd.training.AdamW (got {type(optimizer).__name__})')
        if ops.MULTIPLY != 'f32':
            raise NotImplementedError(f'parameter gradients are formed with the fp32 multiply only (ops.MULTIPLY = {ops.MULTIPLY!r})')
        if rows < 1:
            raise ValueError('GraphedStep: rows >= 1')
        if data is not None and (batch_size is None or batch_size < 1):
            raise ValueError('GraphedStep(data=...): batch_size >= 1')
        if data is None and batch_size is not None:
            raise ValueError('GraphedStep: batch_size goes with data=')
        self.sde, self.opt, self.c, self.rows = sde, optimizer, c, int(rows)
        self.data, self.batch_size = data, batch_size
        self._route = dict(mlp=bool(mlp), wgrad=_check_route(wgrad), net1d=bool(net1d))
        self.device = next(sde.parameters()).device
        if data is not None and data.data.device != self.device:
            raise ValueError(f'GraphedStep(data=...): the dataset lives on {data.data.device}, the net on {self.device}')
        self._ctr = torch.zeros(2, device=self.device, dtype=torch.int64)          # {training step of the keyed draws, table row}
        self.noise = KeyedLossNoise(seed, counter=self._ctr[0:1])
        self._irow = self._ctr[1:2]
        self.loss_sum = torch.zeros((), device=self.device, dtype=torch.float32)
        self._graph = self._shape = self._x = self._loss = self._cap = None
        self._pending, self._stepped = 0, ()                # steps the optimizer's CPU `step` scalars lag behind, and whose
        self._table = self._table_key = None
        self._row = 0                                       # host mirror of the device row counter
        optimizer.register_state_dict_pre_hook(lambda opt: self.sync_state())
        optimizer.register_load_state_dict_pre_hook(lambda opt, sd: self.sync_state())
        optimizer.register_load_state_dict_post_hook(lambda opt: self._drop_graph())
        optimizer.register_step_pre_hook(lambda opt, args, kwargs: self._before_foreign_step())

    # ------------------------------------------------------------------ optimizer state
    def sync_state(self) -> None:
        """Bring the optimizer's ``state[p]['step']`` CPU scalars up to date."""
        n, self._pending = self._pending, 0
        if n:
            for p in self._stepped:
                self.opt.state[p]['step'] += n

    def _before_foreign_step(self):
        self.sync_state()
        self._table_key = None                              # (its step advances the counts: the table's rows no longer match)

    def _drop_graph(self) -> None:
        self._graph = self._shape = self._cap = None
        self._table_key = None

    def _buckets(self):
        """[(group, [(parameter, gradient, state)])] per (param group, step count), as ``AdamW.step`` forms them; creates missing state."""
        out = []
        for group in self.opt.param_groups:
            self.opt._check_group(group)
            buckets = {}
            for p in group['params']:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                state = self.opt.state[p]
                if len(state) == 0:
                    state = self.opt._init_state(p)
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous():
                    raise ValueError('sda_amd.training.GraphedStep: gradients are dense contiguous fp32 tensors on the parameter\'s device')
                buckets.setdefault(float(state['step']), []).append((p, g, state))
            out += [(group, items) for items in buckets.values()]
        return out

    # ------------------------------------------------------------------ the scalar table
    @staticmethod
    def _baked(buckets):
        """What a captured launch holds by value."""
        return tuple((tuple(g['betas']), g['eps']) for g, _items in buckets)

    def _table_for(self, buckets) -> None:
        """The device table [len(buckets) * rows][3]: block b holds {decay, step_size, rsqrt_bc2} of the next ``rows`` steps of bucket b
        at its group's current hyper-parameters (``step_scalars``, as ``AdamW._launch``).  Rebuilt -- pinned upload and a reset of the
        device row counter, both in stream order: no synchronisation -- when the rows ran out or a hyper-parameter changed."""
        key = tuple((float(g['lr']), tuple(g['betas']), g['eps'], g['weight_decay']) for g, _items in buckets)
        if key == self._table_key and self._row < self.rows:
            return
        self.sync_state()
        host = torch.cat([scalar_rows(float(g['lr']), g['betas'], g['weight_decay'], float(items[0][2]['step']), self.rows)
                          for g, items in buckets]).pin_memory()
        if self._table is None or self._table.shape != host.shape:
            self._drop_graph()                              # (a graph points at the old table)
            self._table = torch.empty(host.shape, device=self.device, dtype=torch.float32)
        self._table.copy_(host, non_blocking=True)          # (the pinned block is not reused before the copy ran: torch's host allocator)
        self._irow.zero_()
        self._row, self._table_key = 0, key

    # ------------------------------------------------------------------ packings
    def _other_plans(self):
        """The whole-MLP plans of the net whose slabs the optimizer launch does NOT write (an ``AdamW`` made without ``net=``)."""
        from . import mlp
        from .nn import ResMLP
        if self.opt._mlps:
            self.opt._plan_slots()
        covered, others = self.opt._plans, []
        for m in self.sde.modules():
            if isinstance(m, ResMLP):
                layers = list(m)
                if all(isinstance(l, torch.nn.Linear) or mlp._is_res_block(l) for l in layers):
                    plan = mlp._fused_plan(layers)
                    if plan is not None and not any(plan is q for q in covered):
                        others.append(plan)
        return others

    def _stale_packs(self) -> None:
        """Make every packing the step reads and the optimizer launch does not write stale: its re-pack launches then belong to the body
        (the convolution caches of the U-Net routes, net1d's pack launch, plans outside ``AdamW(net=...)``)."""
        for m in self.sde.modules():
            f = getattr(m, 'invalidate_engine', None)
            if f is not None:
                f()
        for plan in self._other_plans():
            plan._key = None

    # ------------------------------------------------------------------ one step
    def _body(self, x, build_table: bool):
        """loss, backward, the optimizer launches, loss_sum and the counters -> (loss, buckets, plans).  Gradients are None on entry.
        With ``data=``: ``x`` is the static input to draw the next batch into, or None (an uncaptured batch of its own storage)."""
        from . import ops
        if self.data is not None:
            x = self.data.draw(self.batch_size, out=x)
        had, prev = 'loss_noise' in self.sde.__dict__, self.sde.__dict__.get('loss_noise')
        self.sde.loss_noise = self.noise
        try:
            with torch.enable_grad(), parameter_gradients(**self._route):
                loss = self.sde.loss(x, self.c)
            loss.backward()
        finally:
            if had:
                self.sde.loss_noise = prev
            else:
                del self.sde.loss_noise
        with torch.no_grad():
            buckets = self._buckets()
            if build_table:
                self._table_for(buckets)
            if self._table is None or self._table.shape[0] != len(buckets) * self.rows or self._row >= self.rows:
                raise RuntimeError('GraphedStep: the scalar table does not match the step (the set of trained parameters changed)')
            slots = self.opt._plan_slots() if self.opt._mlps else {}
            plans = {}
            with torch.cuda.device(self.device):
                for b, (group, items) in enumerate(buckets):
                    descs, pl = self.opt._descriptors(group, items, slots)
                    plans.update(pl)
                    block = self._table[b * self.rows:(b + 1) * self.rows]
                    for d in descs:
                        ops.adamw_step_dev(d, block, self._irow)
            loss = loss.detach()
            self.loss_sum += loss
            self._ctr += 1
        return loss, buckets, plans

    def _after(self, buckets, plans) -> None:
        """Host bookkeeping of a finished (or replayed) step: version counters (no launch), the plans' keys -- their slabs hold the new
        values --, the lagging step counts, the row mirror."""
        params = [p for _g, items in buckets for p, _gr, _s in items]
        torch.autograd.graph.increment_version(params)
        for plan in plans.values():
            plan._key = plan._pack_key()
        self._stepped = params
        self._pending += 1
        self._row += 1

    def _clear_grads(self) -> None:
        for group in self.opt.param_groups:
            for p in group['params']:
                p.grad = None

    def _eager(self, x):
        self.sync_state()                                   # (the buckets are keyed on the step counts)
        self._clear_grads()
        loss, buckets, plans = self._body(x if self.data is not None else x.contiguous(), build_table=True)
        self._after(buckets, plans)
        self._clear_grads()
        return loss, buckets

    def _capture(self, x):
        dev = self.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up off the capture stream: a real step (packs weights, sizes pools)
            loss, buckets = self._eager(x)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.sync_state()
        self._table_for(buckets)                            # (a fresh table where the warm-up used its last row: never inside the capture)
        if self.data is not None:
            self._x = torch.empty(self.data.batch_shape(self.batch_size), device=self.device, dtype=torch.float32)
        else:
            self._x = x.contiguous().clone()
        self._stale_packs()
        torch.cuda.synchronize(dev)
        from . import ops
        graph = torch.cuda.CUDAGraph()
        try:
            with ops.capture_without_gc(), torch.cuda.graph(graph):    # (gradients are None: backward allocates them from the graph's pool)
                static_loss, cap_buckets, plans = self._body(self._x, build_table=False)
        finally:
            # nothing ran: the packings the capture made "current" are not (outside consumers re-pack; the graph re-packs at its head)
            self._stale_packs()
        self._graph, self._shape, self._loss = graph, tuple(self._x.shape), static_loss
        # what the graph's launches point at: the buckets (parameters, pool gradients, moments) and the slabs the optimizer launch writes
        self._cap = (cap_buckets, plans, self._baked(cap_buckets), [(plan, plan.wf, plan.wb, plan.bias) for plan in plans.values()])
        return loss

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """One training step on the batch ``x`` (with ``data=``: on the dataset's next batch, ``x`` is not given) -> the 0-dim loss (the
        graph's static tensor once captured: valid until the next step)."""
        if (x is None) != (self.data is not None):
            raise TypeError('GraphedStep.step: a batch x without data=, no argument with data=')
        if self.data is not None:
            shape = self.data.batch_shape(self.data.rows(self.batch_size))
            full = shape[0] == self.batch_size
        else:
            shape, full = tuple(x.shape), True
        if self._graph is not None and self._baked(self._cap[0]) != self._cap[2]:
            self._drop_graph()
        if self._graph is not None and shape == self._shape:
            self._table_for(self._cap[0])                   # (drops the graph if the table had to move)
        if self._graph is None and full:
            return self._capture(x)
        if self._graph is None or shape != self._shape:
            return self._eager(x)[0]
        buckets, plans, _baked, slabs = self._cap
        for plan, wf, wb, bias in slabs:                    # a parameter changed from outside: re-pack INTO the slabs the graph points at
            if plan._key != plan._pack_key() or plan.wf is not wf:
                plan._pack()
                if plan.wf is not wf:
                    wf.copy_(plan.wf); wb.copy_(plan.wb); bias.copy_(plan.bias)
                    plan.wf, plan.wb, plan.bias = wf, wb, bias
        if self.data is None:
            self._x.copy_(x)
        self._graph.replay()
        if self.data is not None:
            self.data.replayed()
        self._after(buckets, plans)
        return self._loss
