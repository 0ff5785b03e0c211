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
kernels of the samplers stay sampling-only.  ``sda_amd.utils.loop`` switches both on."""
import contextlib
import threading

import torch

SUPPORTED = ('ScoreUNet (and subclasses such as LocalScoreUNet) with spatial = 1 or 2, alone, in MCScoreNet or in MCScoreWrapper, '
             "with the fp32 multiply (ops.MULTIPLY == 'f32')")

SUPPORTED_MLP = ('ScoreNet (TimeEmbedding + ResMLP of Linear layers and LayerNorm residual blocks: widths <= 256, biases present, one '
                 'activation, one LayerNorm eps), alone or as the kernel of MCScoreNet, on the device, '
                 "with the fp32 multiply (ops.MULTIPLY == 'f32'), under parameter_gradients(mlp=True)")

_enabled = False
_mlp = False
_local = threading.local()


def enable(mlp: bool = False) -> None:
    """Form parameter gradients in the U-Net backward from now on; ``mlp=True``: in the ScoreNet / ResMLP backward as well."""
    global _enabled, _mlp
    _enabled, _mlp = True, bool(mlp)


def disable() -> None:
    """Back to the default: input gradients only."""
    global _enabled, _mlp
    _enabled, _mlp = False, False


def enabled() -> bool:
    return _enabled


def mlp_enabled() -> bool:
    """Are parameter gradients of ScoreNet / ResMLP switched on (the second opt-in)?"""
    return _enabled and _mlp


@contextlib.contextmanager
def parameter_gradients(on: bool = True, mlp: bool = False):
    """Switch parameter gradients on (or off) inside the block, those of ScoreNet / ResMLP with ``mlp=True``; the previous state of
    both switches is restored on exit."""
    global _enabled, _mlp
    prev = (_enabled, _mlp)
    _enabled, _mlp = bool(on), bool(on) and bool(mlp)
    try:
        yield
    finally:
        _enabled, _mlp = prev


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
