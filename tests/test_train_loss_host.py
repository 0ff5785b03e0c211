"""CPU: the entry points of the replayed training step (csrc/train_loss.hip, sda_adamw_step_dev in csrc/optim.hip; sda_amd.training).

The refusals of sda_loss_perturb / sda_loss_mse / sda_adamw_step_dev without a GPU, the table-reading optimizer launch through the host
emulator against the by-value one, and the host table builder against the scalars AdamW._launch passes.  The device tests are
tests/test_gpu_train_loss.py and tests/test_gpu_graphed_step.py."""
import ctypes
import math

import pytest
import torch

from sda_amd import _lib, training
from sda_amd import build as sbuild
from tests import adamw_ref as A
from tests import loss_ref as R

BADARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def lib():
    sbuild.build()
    return _lib.load()


@pytest.fixture(scope='module')
def emu():
    e = A.load_emu()
    e.sda_adamw_step_dev_emulate.restype = ctypes.c_int
    e.sda_adamw_step_dev_emulate.argtypes = [ctypes.POINTER(_lib.AdamWDesc), ctypes.c_void_p, ctypes.c_void_p]
    return e


def test_abi_version_stays_14(lib):
    assert lib.sda_abi_version() == 14


def test_loss_perturb_rejects_bad_arguments_without_a_gpu(lib):
    x = torch.zeros(4, 8)
    t, eps, xt = torch.zeros(4), torch.zeros(4, 8), torch.zeros(4, 8)

    def call(xp=x.data_ptr(), rows=4, per_row=8, row0=0, step=0, ak=1, sk=0, tp=t.data_ptr(), ep=eps.data_ptr(), xtp=xt.data_ptr()):
        return lib.sda_loss_perturb(xp, rows, per_row, 7, row0, step, None, ak, 1e-3, 1.5, sk, tp, ep, xtp, None)
    for kw in (dict(xp=None), dict(tp=None), dict(ep=None), dict(xtp=None), dict(rows=0), dict(rows=-3), dict(per_row=0), dict(row0=-1),
               dict(step=-1), dict(ak=3), dict(ak=-1), dict(sk=3), dict(sk=-1)):
        assert call(**kw) == BADARG, kw
    assert call(rows=2 ** 31 - 1, per_row=1025) == UNSUPPORTED          # rows * 2 chunks: more than 2^31 - 1 workgroups


def test_loss_mse_rejects_bad_arguments_without_a_gpu(lib):
    a, b, loss, work = torch.zeros(8), torch.zeros(8), torch.zeros(1), torch.zeros(1)

    def call(o=a.data_ptr(), e=b.data_ptr(), n=8, l=loss.data_ptr(), w=work.data_ptr()):
        return lib.sda_loss_mse(o, e, n, l, None, w, None)
    for kw in (dict(o=None), dict(e=None), dict(l=None), dict(w=None), dict(n=0), dict(n=-1)):
        assert call(**kw) == BADARG, kw
    assert lib.sda_loss_mse_plan(0, None, None) == BADARG
    assert lib.sda_loss_mse_plan(2 ** 31 * 4096, None, None) == UNSUPPORTED


@pytest.mark.parametrize('numel', [1, 105, 4096, 4097, 7680, 2 ** 20 + 3, 2 ** 31 + 5])
def test_loss_mse_plan_is_the_documented_geometry(lib, numel):
    blocks, chain = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.sda_loss_mse_plan(numel, ctypes.byref(blocks), ctypes.byref(chain)) == blocks.value
    assert (blocks.value, chain.value) == R.mse_chain(numel)


def test_adamw_step_dev_rejects_bad_arguments_without_a_gpu(lib):
    t = [torch.zeros(8) for _ in range(4)]
    table, irow = torch.zeros(4, 3), torch.zeros(1, dtype=torch.int64)

    def good():
        return A.desc([tuple(t)], 1e-3, 1e-2, 1)
    assert lib.sda_adamw_step_dev(None, table.data_ptr(), irow.data_ptr(), None) == BADARG
    assert lib.sda_adamw_step_dev(ctypes.byref(good()), None, irow.data_ptr(), None) == BADARG
    assert lib.sda_adamw_step_dev(ctypes.byref(good()), table.data_ptr(), None, None) == BADARG          # irow NULL
    for n in (0, 33):
        d = good()
        d.ntensor = n
        assert lib.sda_adamw_step_dev(ctypes.byref(d), table.data_ptr(), irow.data_ptr(), None) == BADARG, n
    d = good()
    d.g[0] = None
    assert lib.sda_adamw_step_dev(ctypes.byref(d), table.data_ptr(), irow.data_ptr(), None) == BADARG
    d = good()
    d.pack_kind[0] = 3
    assert lib.sda_adamw_step_dev(ctypes.byref(d), table.data_ptr(), irow.data_ptr(), None) == BADARG
    W = torch.zeros(4, 257)
    d = A.desc([(W, W, W, W, 1, 4, 257, W, W)], 1e-3, 1e-2, 1)
    assert lib.sda_adamw_step_dev(ctypes.byref(d), table.data_ptr(), irow.data_ptr(), None) == UNSUPPORTED


def _emu_case(seed):
    """Tensors of 1, 5, 1023, 1025 and 4099 elements, one weight slot (47 x 15) and its bias slot, with fixed gradients."""
    gen = torch.Generator().manual_seed(seed)
    plain = [(torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.zeros(n), torch.zeros(n)) for n in (1, 5, 1023, 1025, 4099)]
    c = A.pack_case(15, 47)
    c['W'].copy_(torch.randn(47, 15, generator=gen))
    c['b'].copy_(torch.randn(47, generator=gen))
    slots = [(c['W'], c['gW'], c['mW'], c['vW'], 1, 47, 15, c['fwd'], c['bwd']), (c['b'], c['gb'], c['mb'], c['vb'], 2, 47, 0, c['bias'], None)]
    return plain + slots, c


def test_emulated_table_rows_equal_the_by_value_launch_bitwise(emu):
    """Three consecutive rows of the table through sda_adamw_step_dev_emulate == three sda_adamw_step_emulate calls given the same
    scalars by value: parameters, both moments and the slab destinations, bitwise."""
    lr, wd = 3e-3, 1e-2
    table = training.scalar_rows(lr, A.BETAS, wd, 0.0, 3).contiguous()
    irow = torch.zeros(1, dtype=torch.int64)
    dev_t, dev_c = _emu_case(0)
    val_t, val_c = _emu_case(0)
    for r in range(3):
        d = A.desc(dev_t, 123.0, 0.5, 7)                   # (the three by-value fields hold other numbers: they must not be read)
        irow[0] = r
        assert emu.sda_adamw_step_dev_emulate(ctypes.byref(d), table.data_ptr(), irow.data_ptr()) == 0
        d = A.desc(val_t, 123.0, 0.5, 7)
        d.decay, d.step_size, d.rsqrt_bc2 = (float(v) for v in table[r])
        assert emu.sda_adamw_step_emulate(ctypes.byref(d)) == 0
    for n, (a, b) in enumerate(zip(dev_t, val_t)):
        for k in (0, 2, 3):
            assert torch.equal(a[k], b[k]), (n, k)
        assert not torch.equal(a[0], _emu_case(0)[0][n][0])          # (the step moved the parameter)
    for k in ('fwd', 'bwd', 'bias'):
        assert torch.equal(dev_c[k], val_c[k]), k
    A.check_pack(dev_c)
    assert emu.sda_adamw_step_dev_emulate(ctypes.byref(A.desc(dev_t, lr, wd, 1)), None, irow.data_ptr()) == BADARG
    assert emu.sda_adamw_step_dev_emulate(ctypes.byref(A.desc(dev_t, lr, wd, 1)), table.data_ptr(), None) == BADARG


@pytest.mark.parametrize('lr', [1e-3, 3.7e-4])
def test_table_builder_reproduces_the_launch_scalars_bitwise(lr):
    """scalar_rows (GraphedStep's table) == the fp32 fields AdamW._launch fills for steps 1 ... 5 and 1000 (tests/adamw_ref.hyper restates
    that arithmetic; the ctypes c_float fields round the doubles as the descriptor does)."""
    wd, betas, eps = 1e-2, (0.9, 0.999), 1e-8
    head, far = training.scalar_rows(lr, betas, wd, 0.0, 5), training.scalar_rows(lr, betas, wd, 999.0, 1)
    for t, row in [(t, head[t - 1]) for t in range(1, 6)] + [(1000, far[0])]:
        d = A.hyper(_lib.AdamWDesc(), lr, wd, t, betas, eps)
        want = torch.tensor([d.decay, d.step_size, d.rsqrt_bc2], dtype=torch.float32)
        assert torch.equal(row, want), (t, row, want)
        assert training.step_scalars(lr, betas, wd, float(t)) == (1.0 - lr * wd, lr / (1.0 - betas[0] ** t), 1.0 / math.sqrt(1.0 - betas[1] ** t))


def test_keyed_loss_noise_and_graphed_step_refuse_on_the_host():
    noise = training.KeyedLossNoise(5, row0=2)
    assert (noise.seed, noise.row0, noise.step) == (5, 2, 0)
    noise.step = 4
    assert noise.step == 4
    with pytest.raises(ValueError):
        training.KeyedLossNoise(0, row0=-1)
    net = torch.nn.Linear(2, 2)
    with pytest.raises(TypeError, match='AdamW'):
        training.GraphedStep(net, torch.optim.AdamW(net.parameters()), seed=0)
