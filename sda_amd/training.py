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
``MCScoreNet`` or wrapped by ``MCScoreWrapper``, with the default fp32 multiply.  Anything else raises ``NotImplementedError``."""
import contextlib
import threading

import torch

SUPPORTED = ('ScoreUNet (and subclasses such as LocalScoreUNet) with spatial = 1 or 2, alone, in MCScoreNet or in MCScoreWrapper, '
             "with the fp32 multiply (ops.MULTIPLY == 'f32')")

_enabled = False
_local = threading.local()


def enable() -> None:
    """Form parameter gradients in the U-Net backward from now on."""
    global _enabled
    _enabled = True


def disable() -> None:
    """Back to the default: input gradients only."""
    global _enabled
    _enabled = False


def enabled() -> bool:
    return _enabled


@contextlib.contextmanager
def parameter_gradients(on: bool = True):
    """Switch parameter gradients on (or off) inside the block; the previous state is restored on exit."""
    global _enabled
    prev = _enabled
    _enabled = bool(on)
    try:
        yield
    finally:
        _enabled = prev


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


def check_supported(net: torch.nn.Module) -> None:
    """Raise NotImplementedError unless every trainable parameter ``net`` reaches belongs to a served U-Net."""
    from . import ops
    from .nn import UNet
    from .score import ScoreUNet
    if ops.MULTIPLY != 'f32':
        raise NotImplementedError(f'parameter gradients are formed with the fp32 multiply only (ops.MULTIPLY = {ops.MULTIPLY!r}); '
                                  f'supported: {SUPPORTED}')
    covered = set()
    for mod in net.modules():
        if isinstance(mod, (ScoreUNet, UNet)):
            spatial = mod.network.spatial if isinstance(mod, ScoreUNet) else mod.spatial
            if spatial not in (1, 2):
                raise NotImplementedError(f'parameter gradients of a spatial = {spatial} U-Net are not formed; '
                                          f'supported: {SUPPORTED}')
            covered.update(id(p) for p in mod.parameters())
    for name, p in net.named_parameters():
        if p.requires_grad and id(p) not in covered:
            raise NotImplementedError(f'parameter {name!r} ({type(_owner(net, name)).__name__}) would receive no gradient: '
                                      f'supported: {SUPPORTED}')


def _owner(net: torch.nn.Module, name: str) -> torch.nn.Module:
    mod = net
    for part in name.split('.')[:-1]:
        mod = getattr(mod, part)
    return mod
