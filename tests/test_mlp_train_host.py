"""CPU: the opt-in parameter gradients of ScoreNet / ResMLP (sda_amd.training with mlp = True; csrc/mlp_train.hip).

The switch and what it serves, the C ABI of the two new descriptors, the weight-gradient tiling replayed on the host against float64
(the emulator shares the planner, the block decode, the staging maps, the loaders and the slab-ordered reduction with the gfx950
kernel), and a build-time guard on the new kernels' registers, scratch and LDS.  The device tests are tests/test_gpu_mlp_train.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from sda_amd import build as sbuild
from sda_amd import ops, training
from sda_amd._lib import MlpWgradDesc
from sda_amd.score import MCScoreNet, ScoreNet, VPSDE
from tests import mlp_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sda_hip.h')
sys.path.insert(0, os.path.join(ROOT, 'tools'))

NETS = [lambda: ScoreNet(5, embedding=8, hidden_features=(16,)), lambda: MCScoreNet(3, order=1, embedding=8, hidden_features=(16,))]


# ------------------------------------------------------------------------------------------------------------ the switch

@pytest.mark.parametrize('make', NETS)
def test_mlp_switch_accepts_scorenet(make):
    with training.parameter_gradients(mlp=True):
        assert training.enabled() and training.mlp_enabled()
        training.check_supported(make())
    assert not training.enabled() and not training.mlp_enabled()


@pytest.mark.parametrize('make', NETS)
def test_default_switch_refuses_scorenet_with_todays_text(make):
    net = make()
    with training.parameter_gradients():
        assert training.enabled() and not training.mlp_enabled()
        with pytest.raises(NotImplementedError, match='would receive no gradient') as err:
            training.check_supported(net)
    assert training.SUPPORTED in str(err.value) and 'ScoreUNet' in str(err.value) and 'spatial = 1 or 2' in str(err.value)
    assert 'mlp=True' in str(err.value)                      # (the one trailing hint)
    assert training.SUPPORTED_MLP not in str(err.value)


def test_flags_restore_after_an_exception_and_nest():
    assert not training.enabled() and not training.mlp_enabled()
    with pytest.raises(RuntimeError, match='boom'):
        with training.parameter_gradients(mlp=True):
            raise RuntimeError('boom')
    assert not training.enabled() and not training.mlp_enabled()
    training.enable(mlp=True)
    try:
        assert training.enabled() and training.mlp_enabled()
        with training.parameter_gradients():                 # (the default inside: U-Nets only)
            assert training.enabled() and not training.mlp_enabled()
            with pytest.raises(ValueError):
                with training.parameter_gradients(False):
                    assert not training.enabled() and not training.mlp_enabled()
                    raise ValueError()
            assert training.enabled() and not training.mlp_enabled()
        assert training.enabled() and training.mlp_enabled()
        training.enable()
        assert training.enabled() and not training.mlp_enabled()
    finally:
        training.disable()
    assert not training.enabled() and not training.mlp_enabled()


def test_input_only_wins_over_the_mlp_switch():
    net = ScoreNet(5, embedding=8, hidden_features=(16,))
    with training.parameter_gradients(mlp=True):
        assert training.mlp_active(net.network)
        with training.input_only():
            assert not training.mlp_active(net.network) and not training.active(net.network)
        with torch.no_grad():
            assert not training.mlp_active(net.network)
    assert not training.mlp_active(net.network)


def test_unserved_resmlps_name_the_served_set():
    wide = ScoreNet(5, embedding=8, hidden_features=(257,))
    nobias = ScoreNet(5, embedding=8, hidden_features=(16,), bias=False)
    mixed = ScoreNet(5, embedding=8, hidden_features=(16, 16))
    mixed.network[2][2] = nn.SiLU()                          # (two activations in one chain)
    with training.parameter_gradients(mlp=True):
        for net in (wide, nobias, mixed):
            with pytest.raises(NotImplementedError, match='widths <= 256') as err:
                training.check_supported(net)
            assert training.SUPPORTED_MLP in str(err.value) and 'ScoreUNet' in str(err.value)
        with pytest.raises(NotImplementedError, match='widths <= 256'):
            VPSDE(wide, shape=(5,)).loss(torch.randn(2, 5))


def test_f16x2_multiply_is_refused_for_the_mlp_route():
    net = ScoreNet(5, embedding=8, hidden_features=(16,))
    prev = ops.set_multiply('f16x2')
    try:
        with training.parameter_gradients(mlp=True):
            with pytest.raises(NotImplementedError, match='fp32 multiply') as err:
                VPSDE(net, shape=(5,)).loss(torch.randn(2, 5))
            assert training.SUPPORTED_MLP in str(err.value)
            with pytest.raises(NotImplementedError, match='fp32 multiply') as err:
                training.check_mlp(net.network)
            assert training.SUPPORTED_MLP in str(err.value)
    finally:
        ops.set_multiply(prev)


def test_cpu_tensors_are_refused_by_the_mlp_route():
    net = ScoreNet(5, embedding=8, hidden_features=(16,))
    with training.parameter_gradients(mlp=True):
        with pytest.raises(NotImplementedError, match='on the device') as err:
            net.network(torch.randn(4, 13))
    assert training.SUPPORTED_MLP in str(err.value)


def test_plan_segments_end_in_front_of_every_later_linear():
    from sda_amd import mlp
    net = ScoreNet(5, embedding=8, hidden_features=(64, 128)).network          # Lin, block, Lin, block, Lin, block
    plan = mlp._fused_plan(list(net))
    assert [k for k, *_ in plan.gemms] == [0, 1, 2, 0, 1, 2, 0, 1, 2]
    assert plan.segments == [(0, 3), (3, 6), (6, 9)] and plan.g_ld == 128
    same = ScoreNet(3, embedding=13, hidden_features=(16, 16)).network          # 16 -> 16: no leading Linear
    plan = mlp._fused_plan(list(same))
    assert plan.segments[0][0] == 0 and all(plan.gemms[g0][0] == 0 for g0, _ in plan.segments[1:])
    wide = mlp._fused_plan(list(ScoreNet(15, embedding=32, hidden_features=(256,) * 5).network))
    assert wide.segments == [(0, 11), (11, 14)] and wide.g_ld == 256


# ------------------------------------------------------------------------------------------------------------ C ABI

@pytest.mark.parametrize('mirror,ctype', [('MlpTrainDesc', 'sda_mlp_train_desc'), ('MlpWgradDesc', 'sda_mlp_wgrad_desc')])
def test_new_desc_layouts_match_c(tmp_path, mirror, ctype):
    """sizeof/offsetof of the ctypes mirrors == what gcc sees in the header."""
    from sda_amd import _lib
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
    # the embedded sda_mlp_desc keeps its layout
    if mirror == 'MlpTrainDesc':
        assert Desc.mlp.offset == 0 and Desc.g_save.offset == ctypes.sizeof(_lib.MlpDesc)


def test_abi_version_and_new_symbols_resolve():
    from sda_amd import _lib
    sbuild.build()
    lib = _lib.load()
    assert lib.sda_abi_version() == 14
    for name in ('sda_mlp_bwd_train', 'sda_mlp_wgrad', 'sda_mlp_wgrad_slabs', 'sda_mlp_wgrad_work_floats'):
        assert hasattr(lib, name)


def test_bad_descriptors_are_rejected_without_a_gpu():
    from sda_amd import _lib
    sbuild.build()
    lib = _lib.load()
    BADARG, UNSUPPORTED = -1, -2
    case = R.make_case(16, 15, 16, 0)
    bufs = R.buffers([case])
    work = torch.zeros(4096)
    good = lambda **kw: R.wgrad_desc([case], bufs, work, **kw)
    assert lib.sda_mlp_wgrad_slabs(ctypes.byref(good())) == 1
    assert lib.sda_mlp_wgrad_work_floats(ctypes.byref(good())) == 16 * 16
    assert lib.sda_mlp_wgrad_slabs(None) == UNSUPPORTED
    for field, value, rc in (('rows', 0, UNSUPPORTED), ('ngemm', 0, UNSUPPORTED), ('ngemm', 33, UNSUPPORTED), ('slabs', -1, BADARG),
                             ('slabs', 65, BADARG)):
        d = good()
        setattr(d, field, value)
        assert lib.sda_mlp_wgrad_slabs(ctypes.byref(d)) == rc, field
        assert lib.sda_mlp_wgrad(ctypes.byref(d), None) == rc, field
    d = good()
    d.work = None                                            # the size queries do not ask for the buffer they size; the launch does
    assert lib.sda_mlp_wgrad_slabs(ctypes.byref(d)) == 1 and lib.sda_mlp_wgrad_work_floats(ctypes.byref(d)) == 16 * 16
    assert lib.sda_mlp_wgrad(ctypes.byref(d), None) == BADARG
    for field, value, rc in (('in_f', 257, UNSUPPORTED), ('out_f', 257, UNSUPPORTED), ('out_f', 0, UNSUPPORTED), ('kind', 3, UNSUPPORTED),
                             ('src', None, BADARG), ('g', None, BADARG), ('dw', None, BADARG), ('src_ld', 14, BADARG)):
        d = good()
        getattr(d, field)[0] = value
        assert lib.sda_mlp_wgrad(ctypes.byref(d), None) == rc, field
    d = good()
    d.kind[0], d.mean[0] = 1, None
    assert lib.sda_mlp_wgrad(ctypes.byref(d), None) == BADARG
    d = good()
    d.g_ld = 15
    assert lib.sda_mlp_wgrad(ctypes.byref(d), None) == BADARG
    # sda_mlp_bwd_train: what mlp_check refuses, and the cotangent stream's own arguments
    t = _lib.MlpTrainDesc()
    assert lib.sda_mlp_bwd_train(None, None) == BADARG
    m = t.mlp
    m.rows, m.ngemm, m.act = 4, 2, 1
    m.kind[0], m.in_f[0], m.out_f[0], m.kind[1], m.in_f[1], m.out_f[1] = 1, 16, 16, 2, 16, 16
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    m.w, m.x, m.x_ld, m.out, m.out_ld = p, p, 16, p, 16
    m.a_save, m.z_save, m.save_stride, m.save_ld, m.mean_save, m.rstd_save, m.stat_stride = p, p, 4 * 128, 128, p, p, 4
    t.g_save, t.g_stride, t.g_ld = None, 4 * 16, 16
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == BADARG            # (null g_save)
    t.g_save, t.g_ld = p, 12
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == BADARG            # (a row shorter than the padded width)
    t.g_ld, t.g_stride = 16, 4 * 16 - 4
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == BADARG            # (GEMM stride shorter than the rows)
    t.g_stride = 4 * 16
    m.rows = 0
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == UNSUPPORTED
    m.rows, m.in_f[0] = 4, 257
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == UNSUPPORTED
    m.in_f[0], m.out_f[0], m.in_f[1], m.out_f[1], m.unbiased = 1, 1, 1, 1, 1
    assert lib.sda_mlp_bwd_train(ctypes.byref(t), None) == UNSUPPORTED       # (unbiased LayerNorm of one feature)


# ------------------------------------------------------------------------------------------------------------ the tiling, replayed

@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_mlp_wgrad_emulate.restype = ctypes.c_int
    lib.sda_mlp_wgrad_emulate.argtypes = [ctypes.POINTER(MlpWgradDesc)]
    return R.bind(lib)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('rows', R.ROWS)
def test_wgrad_emulator_matches_float64(emu, rows, shape, kind):
    def run(d):
        assert emu.sda_mlp_wgrad_emulate(ctypes.byref(d)) == 0
    R.check_case(run, emu, R.make_case(rows, shape[0], shape[1], kind))


def test_wgrad_emulator_planner_and_chain(emu):
    """Slab counts are a function of the shapes only (forced counts clip to the 32-row stages; no empty slab); a chain of several GEMMs in
    one descriptor gives each GEMM what it gets alone, bitwise."""
    c = R.make_case(257, 15, 16, 0)
    b = R.buffers([c])
    stages = (257 + 31) // 32
    assert emu.sda_mlp_wgrad_slabs(ctypes.byref(R.wgrad_desc([c], b, slabs=0))) == stages             # (1 tile: 1024 blocks wanted)
    assert emu.sda_mlp_wgrad_slabs(ctypes.byref(R.wgrad_desc([c], b, slabs=64))) == stages
    assert emu.sda_mlp_wgrad_slabs(ctypes.byref(R.wgrad_desc([c], b, slabs=7))) == 5                  # (ceil(9 / 7) = 2 stages per slab)
    assert emu.sda_mlp_wgrad_slabs(ctypes.byref(R.wgrad_desc([c], b, slabs=2))) == 2
    cases = [R.make_case(65, i, 16, k, act='GELU', seed=s) for s, (i, k) in enumerate(((47, 0), (16, 1), (16, 2), (129, 0)))]
    alone = []
    for cs in cases:
        bufs = R.buffers([cs])
        work = torch.full((emu.sda_mlp_wgrad_work_floats(ctypes.byref(R.wgrad_desc([cs], bufs, slabs=2))),), float('nan'))
        assert emu.sda_mlp_wgrad_emulate(ctypes.byref(R.wgrad_desc([cs], bufs, work, slabs=2))) == 0
        alone.append(bufs[0])
    bufs = R.buffers(cases)
    work = torch.full((emu.sda_mlp_wgrad_work_floats(ctypes.byref(R.wgrad_desc(cases, bufs, slabs=2))),), float('nan'))
    assert emu.sda_mlp_wgrad_emulate(ctypes.byref(R.wgrad_desc(cases, bufs, work, slabs=2))) == 0
    assert not torch.isnan(work).any()                       # (work is exactly the partials: no gap, nothing beyond)
    for cs, one, got in zip(cases, alone, bufs):
        n = cs['out_f'] * cs['in_f']
        assert torch.equal(one[0][:n], got[0][:n]) and torch.equal(one[1][:cs['out_f']], got[1][:cs['out_f']])
        assert torch.isnan(got[0][n:]).all() and torch.isnan(got[1][cs['out_f']:]).all()
        from tests.util import rel_err
        assert rel_err(got[0][:n].reshape(cs['out_f'], cs['in_f']), cs['dw64']) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ build-time guard

def test_train_kernels_no_spills_no_scratch_lds_budget():
    """The VJP kernels with cotangent streams keep what tests/test_isa_guard_mlp.py holds for mlp1d.o's VJP kernels, whose text they are
    (csrc/mlp1d_vjp_kernels.hpp, included by both units): no spill, no scratch instruction, 512 registers (one wave per SIMD), LDS within
    160 KiB with the launch's dynamic part; the weight-gradient kernels likewise."""
    import isa_guard as G
    sbuild.build()
    obj = os.path.join(ROOT, 'sda_amd', 'lib', 'mlp_train.o')
    md, dis = G.kernel_metadata(obj), G.disassemble(obj)
    dyn = (2 * 8 * 8 * 256 + 4096) * 4                       # sda_mlp_bwd_train: two unit buffers + the bias region
    vjp = sorted(n for n in md if 'mlp_train_vjp_kernel' in n)
    wg = sorted(n for n in md if 'mlp_wgrad_kernel' in n or 'mlp_wgrad_reduce_kernel' in n)
    assert len(vjp) == 2 and sum('_wide' in n for n in vjp) == 1 and len(wg) == 2, (vjp, wg)
    assert not [n for n in md if 'mlp_fwd_kernel' in n or 'mlp_bwd_kernel' in n]      # (those names are mlp1d.o's, pinned there)
    for n in vjp + wg:
        k, ins = md[n], dis[n]
        assert k['vgpr_spill_count'] == 0, (n, k)
        assert not [i for i in ins if 'scratch_' in i], n
        assert k['group_segment_fixed_size'] + (dyn if n in vjp else 0) <= 160 * 1024, (n, k)
        assert k['vgpr_count'] <= 512, (n, k)
    for n in vjp + [x for x in wg if 'reduce' not in x]:
        assert sum(1 for i in dis[n] if 'v_mfma_f32' in i) > 0, n


def test_train_vjp_kernels_multiply_as_the_mlp1d_vjp_kernels_do():
    """One VJP text, two units: the training kernels issue the fp32 MFMAs of mlp_bwd_kernel<false> / mlp_bwd_kernel_wide<false>, both counts
    read from the built objects (the pinned numbers are tests/test_isa_guard_mlp.py's alone)."""
    import isa_guard as G
    sbuild.build()
    train = G.disassemble(os.path.join(ROOT, 'sda_amd', 'lib', 'mlp_train.o'))
    mlp1d = G.disassemble(os.path.join(ROOT, 'sda_amd', 'lib', 'mlp1d.o'))

    def mfmas(dis, pick):
        names = [n for n in dis if pick(n)]
        assert len(names) == 1, names
        return sum(1 for i in dis[names[0]] if 'v_mfma_f32_16x16x4' in i)

    narrow = mfmas(train, lambda n: 'mlp_train_vjp_kernel' in n and '_wide' not in n)
    wide = mfmas(train, lambda n: 'mlp_train_vjp_kernel' in n and '_wide' in n)
    assert narrow > 0 and wide > 0
    assert narrow == mfmas(mlp1d, lambda n: 'mlp_bwd_kernelILb0E' in n)
    assert wide == mfmas(mlp1d, lambda n: 'mlp_bwd_kernel_wideILb0E' in n)
