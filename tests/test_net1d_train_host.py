"""CPU: the host replays of csrc/net1d_train.hip (libsda_emu.so) -- the one-launch weight gradient of a single-level 1-D U-Net with its
slab planner and ordered reduction, and the one-launch weight pack -- against float64 / numpy restatements, and the ``net1d`` switch of
sda_amd.training through the Python orchestration (tests/cpu_shim.py)."""
import ctypes

import numpy as np
import pytest
import torch

from sda_amd import build as sbuild
from sda_amd import training
from sda_amd._lib import Net1dPackDesc, Net1dWgradDesc
from tests import net1d_train_ref as R


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    for name, res, arg in (('sda_net1d_wgrad_emulate', ctypes.c_int, Net1dWgradDesc), ('sda_net1d_wgrad_slabs', ctypes.c_int, Net1dWgradDesc),
                           ('sda_net1d_wgrad_work_floats', ctypes.c_int64, Net1dWgradDesc), ('sda_net1d_pack_emulate', ctypes.c_int, Net1dPackDesc)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, [ctypes.POINTER(arg)]
    return lib


def _run(emu, t, slabs=0, frozen=()):
    return R.run_wgrad(t, emu.sda_net1d_wgrad_work_floats, lambda d: emu.sda_net1d_wgrad_emulate(ctypes.byref(d)), slabs, frozen)


def _cfg(circular, c, cin, cout, nb, n, length, channel_last, per_image, unbiased, act):
    return dict(circular=circular, c=c, cin=cin, cout=cout, nb=nb, n=n, len=length, channel_last=channel_last, per_image=per_image,
                unbiased=unbiased, act=act)


# both paddings, c in {8, 48, 64}, cin / cout in {1, 3, 5}, nblocks in {0, 1, 6}, (B, L, C) and planar input, shared and per-image
# modulation, both variance conventions, every activation id the kernels take (0 .. 5)
CASES = [
    _cfg(False, 8, 1, 1, 0, 2, 16, False, False, 0, 1),
    _cfg(True, 48, 3, 5, 1, 3, 19, True, True, 1, 1),
    _cfg(False, 64, 5, 3, 6, 2, 33, True, True, 1, 1),
    _cfg(True, 64, 3, 3, 1, 5, 7, False, False, 0, 2),
    _cfg(False, 8, 5, 1, 1, 2, 9, False, True, 1, 3),
    _cfg(True, 48, 1, 5, 1, 1, 40, True, False, 0, 4),
    _cfg(False, 8, 3, 3, 1, 2, 12, False, True, 1, 5),
    _cfg(True, 8, 3, 3, 1, 2, 12, False, True, 0, 0),
]


@pytest.mark.parametrize('i', range(len(CASES)))
def test_replay_matches_float64(emu, i):
    t = R.random_saved(CASES[i], seed=40 + i)
    R.check_against(R.reference_grads(t), _run(emu, t), what=f'case {i}')


def test_slabs(emu):
    cfg = CASES[2]
    t = R.random_saved(cfg, seed=7)
    d1, _, k1 = R.wgrad_desc(t)
    planned = emu.sda_net1d_wgrad_slabs(ctypes.byref(d1))
    assert planned > 1, planned                              # (66 rows = 3 stages: one slab each)
    # a function of the shapes only: other tensors, no tensors at all
    d2, _, k2 = R.wgrad_desc(R.random_saved(cfg, seed=8))
    assert emu.sda_net1d_wgrad_slabs(ctypes.byref(d2)) == planned
    bare = Net1dWgradDesc()
    for f in ('n', 'len', 'cin', 'c', 'cout', 'nblocks', 'circular', 'act'):
        setattr(bare.net, f, getattr(d1.net, f))
    assert emu.sda_net1d_wgrad_slabs(ctypes.byref(bare)) == planned
    assert emu.sda_net1d_wgrad_work_floats(ctypes.byref(bare)) == emu.sda_net1d_wgrad_work_floats(ctypes.byref(d1))
    ref = R.reference_grads(t)
    runs = {}
    for slabs in (0, 1, 64):
        a, b = _run(emu, t, slabs), _run(emu, t, slabs)
        R.check_against(ref, a, what=f'slabs {slabs}')
        for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
            assert torch.equal(x, y), f'slabs {slabs}: not reproducible'
        runs[slabs] = a
    # a forced count beyond the stages is capped, a negative or too large one refused
    d1.slabs = 64
    assert emu.sda_net1d_wgrad_slabs(ctypes.byref(d1)) == 3
    for bad in (-1, 65):
        d1.slabs = bad
        assert emu.sda_net1d_wgrad_slabs(ctypes.byref(d1)) == -1


def test_frozen_outputs_are_skipped(emu):
    t = R.random_saved(CASES[1], seed=9)
    full = _run(emu, t)
    part = _run(emu, t, frozen=(0, 2))
    for v in (1, 3):
        assert torch.equal(full[0][v], part[0][v]) and torch.equal(full[1][v], part[1][v])
    assert torch.equal(full[2], part[2])


def test_unsupported_and_bad_arguments(emu):
    t = R.random_saved(CASES[0], seed=1)
    d, _, keep = R.wgrad_desc(t)
    d.net.c = 65
    assert emu.sda_net1d_wgrad_slabs(ctypes.byref(d)) == -2
    d.net.c, d.net.nblocks = 8, 9
    assert emu.sda_net1d_wgrad_slabs(ctypes.byref(d)) == -2
    d.net.nblocks = 0
    assert emu.sda_net1d_wgrad_emulate(ctypes.byref(d)) == -1            # no work buffer


def _numpy_packs(ws, bs, cin_keep):
    """The per-convolution packings of the documented [3][64][64] layout (include/sda_hip.h, sda_net1d_desc)."""
    nconv = len(ws)
    wf, wb, bias = np.zeros((nconv, 3, 64, 64), np.float32), np.zeros((nconv, 3, 64, 64), np.float32), np.zeros((nconv, 64), np.float32)
    for v, w in enumerate(ws):
        w = w.numpy()
        cout, cin = w.shape[:2]
        wf[v, :, :cin, :cout] = w.transpose(2, 1, 0)                      # [tap][ci][co]
        if bs[v] is not None:
            bias[v, :cout] = bs[v].numpy()
    for s, v in enumerate(reversed(range(nconv))):                       # tail^T, (conv2^T, conv1^T) of the blocks in reverse, head^T
        w = ws[v].numpy()
        cout, cin = w.shape[:2]
        keep = min(cin, cin_keep) if v == 0 else cin
        wb[s, :, :cout, :keep] = w[:, :keep, ::-1].transpose(2, 0, 1)    # [tap][co][ci], taps reversed
    return wf, wb, bias


@pytest.mark.parametrize('cin,c,cout,nb,keep', [(3, 64, 3, 6, 3), (5, 48, 1, 0, 2), (1, 8, 5, 1, 1), (3, 8, 3, 2, 0)])
def test_pack_replay_is_the_documented_permutation(emu, cin, c, cout, nb, keep):
    g = torch.Generator().manual_seed(3)
    shapes = [(c, cin)] + [(c, c)] * (2 * nb) + [(cout, c)]
    ws = [torch.randn(o, i, 3, generator=g) for o, i in shapes]
    bs = [None if v == 1 else torch.randn(o, generator=g) for v, (o, _) in enumerate(shapes)]
    nconv = len(ws)
    wf, wb, bias = (torch.full((nconv + 1, 3 * 64 * 64), 7.0) for _ in range(2)), None, torch.full((nconv + 1, 64), 7.0)
    wf, wb = wf
    p = R.pack_desc(ws, bs, cin, c, cout, keep, wf, wb, bias)
    assert emu.sda_net1d_pack_emulate(ctypes.byref(p)) == 0
    ef, eb, ebias = _numpy_packs(ws, bs, keep)
    assert np.array_equal(wf[:nconv].numpy().reshape(ef.shape), ef)
    assert np.array_equal(wb[:nconv].numpy().reshape(eb.shape), eb)
    assert np.array_equal(bias[:nconv].numpy(), ebias)
    assert (wf[nconv] == 7).all() and (wb[nconv] == 7).all() and (bias[nconv] == 7).all()
    # one direction at a time, as the engine asks for them
    wb2 = torch.full_like(wb, 7.0)
    assert emu.sda_net1d_pack_emulate(ctypes.byref(R.pack_desc(ws, bs, cin, c, cout, keep, None, wb2, None))) == 0
    assert torch.equal(wb2, wb)
    p.w[1] = None
    assert emu.sda_net1d_pack_emulate(ctypes.byref(p)) == -1


@pytest.mark.parametrize('mirror,ctype', [('Net1dTrainDesc', 'sda_net1d_train_desc'), ('Net1dWgradDesc', 'sda_net1d_wgrad_desc'),
                                          ('Net1dPackDesc', 'sda_net1d_pack_desc')])
def test_desc_layouts_match_c(tmp_path, mirror, ctype):
    import subprocess
    from sda_amd import _lib
    from tests.test_abi_and_host import HEADER
    Desc = getattr(_lib, mirror)
    fields = [f[0] for f in Desc._fields_]
    src = tmp_path / 'layout.c'
    prints = '\n'.join(f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(){{printf("size %zu\\n", '
                   f'sizeof({ctype}));\n{prints}\nreturn 0;}}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', str(src), '-o', str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out['size']) == ctypes.sizeof(Desc)
    for f in fields:
        assert int(out[f]) == getattr(Desc, f).offset, f


# ------------------------------------------------------------------------------------------------ the switch

def test_switch_default_and_restore():
    assert not training.enabled() and not training.net1d_enabled()
    with training.parameter_gradients(mlp=True, wgrad='tiled', net1d=True):
        assert training.enabled() and training.mlp_enabled() and training.wgrad_route() == 'tiled' and training.net1d_enabled()
        with training.parameter_gradients():
            assert training.enabled() and not training.mlp_enabled() and training.wgrad_route() == 'general' and not training.net1d_enabled()
        with training.parameter_gradients(on=False, net1d=True):
            assert not training.enabled() and not training.net1d_enabled()
        assert training.mlp_enabled() and training.wgrad_route() == 'tiled' and training.net1d_enabled()
    assert not training.enabled() and not training.mlp_enabled() and training.wgrad_route() == 'general' and not training.net1d_enabled()
    training.enable(net1d=True)
    try:
        assert training.enabled() and training.net1d_enabled() and not training.mlp_enabled()
    finally:
        training.disable()
    assert not training.enabled() and not training.net1d_enabled()


def test_loop_switches_net1d_on_only_while_steps_run():
    import inspect
    from sda_amd import utils
    assert inspect.signature(utils.loop).parameters['net1d'].default is False
    seen = []

    class Sde(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.ones(()))

        def loss(self, x):
            seen.append((torch.is_grad_enabled(), training.net1d_enabled()))
            return (self.p * x).square().mean()

    data = [(torch.ones(2), {}) for _ in range(4)]
    next(utils.loop(Sde(), data, data, epochs=1, batch_size=2, net1d=True))
    assert (True, True) in seen and (False, False) in seen and (False, True) not in seen      # (validation runs outside the block)
    assert not training.net1d_enabled()
    seen.clear()
    next(utils.loop(Sde(), data, data, epochs=1, batch_size=2))
    assert seen and not any(on for _, on in seen)


def test_a_declined_net_keeps_the_per_layer_route(monkeypatch):
    """Under the switch a net the whole-net plan declines (here: every net -- the shim has no whole-net kernel, as a multi-level or a
    2-D net has none on the device) trains on the per-layer route, silently, with the gradients of the default route."""
    from sda_amd import ops
    from sda_amd.score import VPSDE
    from tests import cpu_shim
    from tests.util import build_unet1d_tiny, load_golden
    cpu_shim.install(monkeypatch)
    _, grp = load_golden('unet1d_tiny')
    net = build_unet1d_tiny()
    net.load_state_dict(grp['sd'])
    called = []
    for name in ('net1d_fwd_train', 'net1d_bwd_train', 'net1d_wgrad', 'net1d_pack'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: called.append(_n))
    sde = VPSDE(net, shape=(16, 3))
    x = torch.randn(4, 16, 3, generator=torch.Generator().manual_seed(2))
    grads = []
    for kw in ({}, dict(net1d=True)):
        net.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        with training.parameter_gradients(**kw):
            sde.loss(x).backward()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    assert not called, called
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
