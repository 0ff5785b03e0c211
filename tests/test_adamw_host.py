"""CPU: the fused AdamW step that keeps the ResMLP weight slabs packed (csrc/optim.hip; sda_amd.training.AdamW).

The C ABI of the descriptor, the refusals of the entry point, the slab position and the arithmetic through the host emulator (it runs
the per-thread function of the gfx950 kernel), the optimizer's state_dict against torch.optim.AdamW, the refused options and a
build-time guard on the kernel's registers and scratch.  The device tests are tests/test_gpu_adamw.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from sda_amd import _lib, training
from sda_amd import build as sbuild
from tests import adamw_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sda_hip.h')
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def emu():
    return A.load_emu()


# ------------------------------------------------------------------------------------------------------------ ABI

def test_adamw_desc_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == what gcc sees in the header; the struct travels by value as a kernel argument."""
    Desc, ctype = _lib.AdamWDesc, 'sda_adamw_desc'
    fields = [f[0] for f in Desc._fields_]
    src = tmp_path / 'layout.c'
    prints = '\n'.join(f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(){{printf("size %zu\\n", '
                   f'sizeof({ctype}));\nprintf("maxt %d\\n", SDA_ADAMW_MAXT);\n{prints}\nreturn 0;}}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', str(src), '-o', str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out['size']) == ctypes.sizeof(Desc) <= 4096
    assert int(out['maxt']) == _lib.ADAMW_MAXT == 32
    for f in fields:
        assert int(out[f]) == getattr(Desc, f).offset, f


def test_bad_descriptors_are_rejected_without_a_gpu():
    sbuild.build()
    lib = _lib.load()
    BADARG, UNSUPPORTED = -1, -2
    assert lib.sda_abi_version() == 14
    assert lib.sda_adamw_step(None, None) == BADARG
    t = [torch.zeros(8) for _ in range(4)]

    def good():
        return A.desc([tuple(t)], 1e-3, 1e-2, 1)
    for n in (0, 33, -1):
        d = good()
        d.ntensor = n
        assert lib.sda_adamw_step(ctypes.byref(d), None) == BADARG, n
    for field in ('p', 'g', 'm', 'v'):
        d = good()
        getattr(d, field)[0] = None
        assert lib.sda_adamw_step(ctypes.byref(d), None) == BADARG, field
    W = torch.zeros(4, 257)
    for out_f, in_f in ((4, 257), (257, 4)):
        d = A.desc([(W, W, W, W, 1, out_f, in_f, W, W)], 1e-3, 1e-2, 1)
        assert lib.sda_adamw_step(ctypes.byref(d), None) == UNSUPPORTED, (out_f, in_f)
    d = A.desc([(t[0], t[1], t[2], t[3], 1, 4, 2, t[0], None)], 1e-3, 1e-2, 1)          # a weight without its transposed slab
    assert lib.sda_adamw_step(ctypes.byref(d), None) == BADARG
    d = A.desc([(t[0], t[1], t[2], t[3], 1, 4, 3, t[0], t[0])], 1e-3, 1e-2, 1)           # numel != out_f in_f
    assert lib.sda_adamw_step(ctypes.byref(d), None) == BADARG
    d = good()
    d.pack_kind[0] = 3
    assert lib.sda_adamw_step(ctypes.byref(d), None) == BADARG


# ------------------------------------------------------------------------------------------------------------ slab position

@pytest.mark.parametrize('in_f,out_f', A.PACK_SHAPES, ids=lambda v: str(v))
def test_emulated_pack_matches_the_host_packer(emu, in_f, out_f):
    """One emulated step with lr = 0 and wd = 0 (p unchanged) from zeroed slabs: the forward destination is mlp._slab(W), the transposed
    one mlp._slab(W.t()), bitwise and padding included; the bias lands in its padded row."""
    c = A.pack_case(in_f, out_f)
    W0, b0 = c['W'].clone(), c['b'].clone()
    assert emu.sda_adamw_step_emulate(ctypes.byref(A.pack_desc(c, 0.0, 0.0))) == 0
    assert torch.equal(c['W'], W0) and torch.equal(c['b'], b0)
    A.check_pack(c)


def test_emulated_pack_of_an_unaligned_weight(emu):
    """A weight whose numel is a multiple of 4 but whose storage starts 4 bytes off a 16-byte boundary takes the scalar path."""
    c = A.pack_case(64, 128)
    for k in ('W', 'gW', 'mW', 'vW'):
        flat = torch.zeros(c[k].numel() + 1)
        flat[1:] = c[k].reshape(-1)
        c[k] = flat[1:].view(128, 64)
        assert c[k].data_ptr() % 16 == 4
    assert emu.sda_adamw_step_emulate(ctypes.byref(A.pack_desc(c, 0.0, 0.0))) == 0
    A.check_pack(c)


# ------------------------------------------------------------------------------------------------------------ arithmetic

@pytest.mark.parametrize('scale', A.SCALES)
def test_emulated_arithmetic_against_float64(emu, scale):
    """Five steps, lr changing each step, wd = 1e-3, tensors of 1 / 5 / 1023 / 4100 elements, against the float64 replay of the formula;
    the yardstick is torch.optim.AdamW(foreach=False, fused=False) on the same inputs (tests/adamw_ref.py check_against_float64).
    Measured (max error of p to float64 over the four tensors): scale 1: emulator 7.05e-7, torch 7.05e-7; scale 1e-3: emulator 7.28e-7,
    torch 7.28e-7 (|p| up to 4: a few ulp over five steps, the same elements on both)."""
    params, grads = A.arithmetic_inputs(scale)
    got = A.emulate_five_steps(emu, params, grads)
    worst = A.check_against_float64(got, A.torch_adamw(params, grads, fused=False), A.replay64(params, grads))
    print(f'scale {scale}: worst p error {worst[0]:.3e} (torch {worst[1]:.3e})')


# ------------------------------------------------------------------------------------------------------------ the optimizer on the host

def _params(device):
    return [torch.nn.Parameter(torch.zeros(3, 5, device=device)), torch.nn.Parameter(torch.zeros(7, device=device))]


@pytest.mark.parametrize('device', ['cpu', 'meta'])
def test_state_dict_moves_to_torch_adamw_and_back(device):
    ours = training.AdamW(_params(device), lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=3e-2)
    assert isinstance(ours, torch.optim.Optimizer)
    # a stepped state, as our step leaves it: a CPU float32 scalar `step`, exp_avg, exp_avg_sq
    for n, p in enumerate(ours.param_groups[0]['params']):
        ours.state[p] = {'step': torch.tensor(3.0), 'exp_avg': torch.full_like(p, 0.5 + n), 'exp_avg_sq': torch.full_like(p, 0.25 + n)}
    sd = ours.state_dict()
    theirs = torch.optim.AdamW(_params(device))
    theirs.load_state_dict(sd)
    g = theirs.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (2e-3, (0.8, 0.99), 1e-7, 3e-2)
    assert not g['amsgrad'] and not g['maximize'] and not g['capturable'] and not g['differentiable']
    for n, p in enumerate(g['params']):
        st = theirs.state[p]
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert st['step'].dtype == torch.float32 and st['step'].device.type == 'cpu' and float(st['step']) == 3.0
        if device == 'cpu':
            assert torch.equal(st['exp_avg'], torch.full_like(p, 0.5 + n)) and torch.equal(st['exp_avg_sq'], torch.full_like(p, 0.25 + n))
    if device == 'cpu':
        for p in g['params']:
            p.grad = torch.ones_like(p)
        theirs.step()                                        # torch accepts the state as its own
        assert all(float(theirs.state[p]['step']) == 4.0 for p in g['params'])
    back = training.AdamW(_params(device))
    back.load_state_dict(theirs.state_dict())
    g = back.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (2e-3, (0.8, 0.99), 1e-7, 3e-2)
    for p in g['params']:
        st = back.state[p]
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and st['step'].device.type == 'cpu' and st['exp_avg'].shape == p.shape
    # LambdaLR and param groups are the base class's
    sched = torch.optim.lr_scheduler.LambdaLR(back, lr_lambda=lambda e: 0.5)
    assert back.param_groups[0]['lr'] == pytest.approx(1e-3)
    back.add_param_group({'params': _params(device), 'lr': 0.1})
    assert len(back.param_groups) == 2 and back.param_groups[1]['weight_decay'] == 1e-2 and back.param_groups[1]['amsgrad'] is False
    del sched


def test_refused_options_raise_value_error():
    for name in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
        with pytest.raises(ValueError, match=name):
            training.AdamW(_params('cpu'), **{name: True})
    with pytest.raises(ValueError, match='tensor lr'):
        training.AdamW(_params('cpu'), lr=torch.tensor(1e-3))
    # a checkpoint of a torch optimizer that used a refused option: refused at the step, not silently ignored
    theirs = torch.optim.AdamW(_params('cpu'), amsgrad=True)
    ours = training.AdamW(_params('cpu'))
    ours.load_state_dict(theirs.state_dict())
    with pytest.raises(ValueError, match='amsgrad'):
        ours.step()
    # parameters that are not fp32 device tensors: refused when their state would be created (constructing on the host works)
    ours = training.AdamW(_params('cpu'))
    for p in ours.param_groups[0]['params']:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match='fp32 device tensors'):
        ours.step()
    assert all(len(ours.state[p]) == 0 for p in ours.param_groups[0]['params'])


# ------------------------------------------------------------------------------------------------------------ build-time guard

def test_adamw_kernel_no_spills_no_scratch():
    """The descriptor is indexed by a wave-uniform tensor number: it must stay in the kernel-argument segment (scalar loads), not be copied
    to private memory.  From the code object's metadata alone."""
    import isa_guard as G
    sbuild.build()
    md = G.kernel_metadata(os.path.join(ROOT, 'sda_amd', 'lib', 'optim.o'))
    names = [n for n in md if 'adamw_step_kernel' in n]
    assert len(names) == 1, list(md)
    k = md[names[0]]
    assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
    assert k['group_segment_fixed_size'] == 0 and k['vgpr_count'] <= 64, k          # (no LDS; 8 waves per SIMD)
