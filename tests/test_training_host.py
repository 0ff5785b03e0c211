"""CPU: the opt-in switch for parameter gradients (sda_amd.training) and what VPSDE.loss does with it, before any kernel runs."""
import importlib
import sys

import pytest
import torch
import torch.nn as nn

from sda_amd import ops, training
from sda_amd.score import MCScoreNet, MCScoreWrapper, ScoreNet, ScoreUNet, VPSDE


def test_switch_off_by_default_and_loss_still_refuses():
    assert not training.enabled()
    sde = VPSDE(ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=2), shape=(2, 8, 8))
    with pytest.raises(NotImplementedError, match='parameter gradients'):
        sde.loss(torch.randn(3, 2, 8, 8))


def test_enable_disable_and_context_manager_restore():
    assert not training.enabled()
    with training.parameter_gradients():
        assert training.enabled()
        with training.parameter_gradients(False):
            assert not training.enabled()
        assert training.enabled()
    assert not training.enabled()
    training.enable()
    try:
        assert training.enabled()
        with training.parameter_gradients():
            pass
        assert training.enabled()
    finally:
        training.disable()
    assert not training.enabled()
    with pytest.raises(RuntimeError):
        with training.parameter_gradients():
            raise RuntimeError('boom')
    assert not training.enabled()


def test_active_needs_grad_mode_and_trainable_parameters():
    net = ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=2)
    assert not training.active(net)
    with training.parameter_gradients():
        assert training.active(net)
        with torch.no_grad():
            assert not training.active(net)
        with training.input_only():
            assert not training.active(net)
        net.requires_grad_(False)
        assert not training.active(net)


@pytest.mark.parametrize('make', [
    lambda: ScoreNet(5, embedding=8, hidden_features=(16,)),
    lambda: MCScoreNet(3, order=1, embedding=8, hidden_features=(16,)),
    lambda: ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=3),
])
def test_unsupported_nets_name_the_supported_set(make):
    net = make()
    sde = VPSDE(net, shape=(5,))
    with training.parameter_gradients():
        with pytest.raises(NotImplementedError, match='ScoreUNet') as err:
            sde.loss(torch.randn(2, 5))
    assert 'spatial = 1 or 2' in str(err.value)


@pytest.mark.parametrize('make', [
    lambda: ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=2),
    lambda: MCScoreWrapper(ScoreUNet(3, embedding=8, hidden_channels=(8,), hidden_blocks=(1,), activation=nn.SiLU, spatial=1)),
])
def test_supported_nets_pass_the_check(make):
    training.check_supported(make())


def test_f16x2_multiply_is_refused():
    net = ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=2)
    prev = ops.set_multiply('f16x2')
    try:
        with training.parameter_gradients():
            with pytest.raises(NotImplementedError, match='ScoreUNet'):
                VPSDE(net, shape=(2, 8, 8)).loss(torch.randn(2, 2, 8, 8))
    finally:
        ops.set_multiply(prev)


def test_sda_training_resolves_after_install_as_sda():
    import sda_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'sda' or k.startswith('sda.')}
    try:
        sda_amd.install_as_sda()
        mod = importlib.import_module('sda.training')
        assert mod is training
        from sda.utils import loop  # noqa: F401
    finally:
        for k in [k for k in sys.modules if k == 'sda' or k.startswith('sda.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_loop_rejects_unknown_optimizer_and_schedule():
    from sda_amd.utils import loop
    sde = VPSDE(ScoreUNet(2, embedding=8, hidden_channels=(4,), hidden_blocks=(1,), spatial=2), shape=(2, 8, 8))
    with pytest.raises(ValueError):
        next(loop(sde, [], [], optimizer='SGD'))
    with pytest.raises(ValueError):
        next(loop(sde, [], [], scheduler='step'))
