r"""Helpers on the sampling path (subset of the reference's ``sda/utils.py``: ACTIVATIONS and the run-config reader,
sda/utils.py:19-25,40-42; the evaluation metrics ``bpf`` / ``emd`` / ``mmd`` of sda/utils.py:168-263 live in
``sda_amd.metrics`` and are re-exported here under the reference's names; the two config writers the reference's
``experiments/*/train.py`` reach through ``from sda.utils import *`` -- ``random_config`` / ``save_config``, sda/utils.py:28-37 --
are plain host code and kept).  ``loop`` is the reference's training loop (sda/utils.py:89-165: AdamW, a linear / cosine /
exponential LambdaLR schedule, ``(loss_train, loss_valid, lr)`` per epoch); it trains with parameter gradients switched on
(``sda_amd.training``).  The reference's ``TrajectoryDataset`` (an h5py file behind a host ``DataLoader``) has a device-resident
counterpart, ``sda_amd.data.DeviceTrajectories`` (re-exported here): ``loop`` draws its batches on the device, and with ``graph=True``
inside the replayed step; any other dataset object goes through a ``DataLoader`` as in the reference.

``from sda.utils import *`` in the reference's drivers also hands on that module's own imports (sda/utils.py:3-16:
``json``, ``math``, ``torch``, ``Path``, ``Tensor``, the ``typing`` names, everything of ``sda.score`` and, where installed,
``h5py`` -- experiments/lorenz/eval.py reads its observations with it); the same names are importable from here."""

import json
import math  # noqa: F401
import random
from pathlib import Path
from typing import *  # noqa: F401,F403

import torch
from torch import Tensor  # noqa: F401

try:
    import h5py  # noqa: F401  (optional: only the drivers' dataset / observation files need it)
except ImportError:
    pass

from . import training
from .data import DeviceTrajectories  # (the device-resident counterpart of sda.utils.TrajectoryDataset)
from .score import *  # noqa: F401,F403  (sda/utils.py:16)
from .metrics import bpf, emd, mmd  # noqa: F401  (sda.utils.bpf / emd / mmd)

ACTIVATIONS = {
    'ReLU': torch.nn.ReLU,
    'ELU': torch.nn.ELU,
    'GELU': torch.nn.GELU,
    'SELU': torch.nn.SELU,
    'SiLU': torch.nn.SiLU,
}


def load_config(path: Path) -> Dict[str, Any]:
    with open(Path(path) / 'config.json', mode='r') as f:
        return json.load(f)


def save_config(config: Dict[str, Any], path: Path) -> None:
    """Write ``path/config.json``; refuses to overwrite an existing run's file (exclusive create, as sda/utils.py:35-37)."""
    with open(Path(path) / 'config.json', mode='x') as f:
        json.dump(config, f)


def random_config(configs: Dict[str, Sequence[Any]]) -> Dict[str, Any]:
    """One uniformly drawn value per key of a {key: candidates} search space (sda/utils.py:28-32; python's ``random``)."""
    drawn = {}
    for key, values in configs.items():
        drawn[key] = random.choice(values)
    return drawn


def _to(x: Any, **kwargs) -> Any:
    """Move a batch (tensor, or nested tuple / list / dict of them) with ``Tensor.to(**kwargs)``."""
    if torch.is_tensor(x):
        return x.to(**kwargs)
    if isinstance(x, (tuple, list)):
        return type(x)(_to(v, **kwargs) for v in x)
    if isinstance(x, dict):
        return {k: _to(v, **kwargs) for k, v in x.items()}
    return x


_SCHEDULES = {
    'linear': lambda epochs: (lambda t: 1 - t / epochs),
    'cosine': lambda epochs: (lambda t: (1 + math.cos(math.pi * t / epochs)) / 2),
    'exponential': lambda epochs: (lambda t: math.exp(-7 * (t / epochs) ** 2)),
}


def loop(sde: 'VPSDE', trainset, validset, epochs: int = 256, batch_size: int = 64, optimizer: str = 'AdamW',
         learning_rate: float = 1e-3, weight_decay: float = 1e-3, scheduler: str = 'linear', device: str = 'cpu',
         fused: bool = False, wgrad: str = 'general', net1d: bool = False, graph: bool = False, seed: int = 0, **absorb) -> Iterator:
    """Train ``sde`` (its score network) on ``trainset`` and yield ``(loss_train, loss_valid, lr)`` once per epoch.

    As the reference's loop: shuffled DataLoaders whose items are ``(x, kwargs)`` pairs (``kwargs`` go on to ``sde.loss``),
    AdamW over ``sde.parameters()``, the learning rate scaled per epoch by the ``linear`` / ``cosine`` / ``exponential`` factor,
    the mean training loss, the mean validation loss (under ``no_grad``) and the learning rate the epoch ran with.  Parameter
    gradients are switched on (``sda_amd.training.parameter_gradients(mlp=True)``: the U-Nets and ScoreNet) while the training steps run.
    ``fused=True`` takes ``sda_amd.training.AdamW`` (one launch per step, the ResMLP weight slabs stay packed) for ``torch.optim.AdamW``;
    ``wgrad='tiled'`` sends the block convolutions' weight gradients to the tiled kernel, ``wgrad='tiled_ht'`` the stride-2 heads' and
    up-sampling tails' as well; ``net1d=True`` trains a single-level 1-D U-Net on the whole-net kernels (``sda_amd.training``).
    ``graph=True`` (implies ``fused``) replays every training step as one hipGraph (``sda_amd.training.GraphedStep``): the loss draws its
    noise keyed on ``seed`` and the step index instead of torch's generator, and the epoch's mean loss is read back once; the items'
    ``kwargs`` must then be empty.  A ``trainset`` / ``validset`` that is a ``sda_amd.data.DeviceTrajectories`` is iterated with its own
    ``batches(batch_size)`` (keyed shuffle and windows, no host tensor work); with ``graph=True`` the stepper draws from such a
    ``trainset`` inside the graph (``GraphedStep(data=...)``)."""
    from torch.utils.data import DataLoader

    class _Resident:
        """A ``DeviceTrajectories`` as the loop iterates a loader: one epoch of ``(x, {})`` batches per ``iter``."""

        def __init__(self, ds):
            self.ds = ds

        def __iter__(self):
            return self.ds.batches(batch_size)
    loaders = [_Resident(ds) if isinstance(ds, DeviceTrajectories) else DataLoader(ds, batch_size=batch_size, shuffle=True)
               for ds in (trainset, validset)]
    fed = graph and isinstance(trainset, DeviceTrajectories)
    if optimizer != 'AdamW':
        raise ValueError(f'optimizer {optimizer!r} (the loop knows AdamW)')
    if fused or graph:
        opt = training.AdamW(sde.parameters(), lr=learning_rate, weight_decay=weight_decay, net=sde)
    else:
        opt = torch.optim.AdamW(sde.parameters(), lr=learning_rate, weight_decay=weight_decay)
    if scheduler not in _SCHEDULES:
        raise ValueError(f'scheduler {scheduler!r} (expected one of {sorted(_SCHEDULES)})')
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=_SCHEDULES[scheduler](epochs))
    stepper = None
    if graph:
        stepper = training.GraphedStep(sde, opt, seed=seed, mlp=True, wgrad=wgrad, net1d=net1d,
                                       **(dict(data=trainset, batch_size=batch_size) if fed else {}))
        opt._opt_called = True       # (the steps run inside the graph: LambdaLR would warn that optimizer.step() was never called)
    for _ in range(epochs):
        losses_train, losses_valid = [], []
        sde.train()
        if graph:
            stepper.loss_sum.zero_()
            n = trainset.remaining(batch_size) if fed else 0
            for _step in range(n):                           # (the stepper draws its own batches: nothing to hand over)
                stepper.step()
            for batch in () if fed else loaders[0]:
                x, kwargs = _to(batch, device=device)
                if kwargs:
                    raise NotImplementedError(f'loop(graph=True) trains on items without keyword arguments (got {sorted(kwargs)})')
                stepper.step(x)
                n += 1
            losses_train.append(stepper.loss_sum / max(n, 1))
        with training.parameter_gradients(mlp=True, wgrad=wgrad, net1d=net1d):
            for batch in () if graph else loaders[0]:
                x, kwargs = _to(batch, device=device)
                loss = sde.loss(x, **kwargs)
                loss.backward()
                opt.step()
                opt.zero_grad()
                losses_train.append(loss.detach())
        sde.eval()
        with torch.no_grad():
            for batch in loaders[1]:
                x, kwargs = _to(batch, device=device)
                losses_valid.append(sde.loss(x, **kwargs))
        lr = opt.param_groups[0]['lr']
        yield torch.stack(losses_train).mean().item(), torch.stack(losses_valid).mean().item(), lr
        sched.step()
