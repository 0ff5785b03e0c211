"""CPU: the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip) -- its served set, its host replay against float64 and the
``wgrad=`` switch.

The replay in libsda_emu.so shares the planner, the staging walk and element maps (halo, wrap, zero padding, the general kernel's
loader helper), the tap offsets, the MFMA lane maps and the slab-ordered reduction with the gfx950 kernel, and refuses any LDS index
outside the tile.  The device kernel is tested in test_gpu_wgrad3.py.  The bound against float64 is the one test_wgrad_emulator.py
applies to the general kernel's replay (1e-5 of the largest element): same arithmetic class."""
import ctypes

import pytest
import torch

from sda_amd import build as sbuild
from sda_amd import training
from sda_amd._lib import WgradDesc
from tests.util import rel_err
from tests.wgrad3_cases import CASES, build
from tests.wgrad_ref import make_case, reference, wgrad_desc

TOL = 1e-5


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    for name, res in (('sda_conv_wgrad3_emulate', ctypes.c_int), ('sda_conv_wgrad3_serves', ctypes.c_int),
                      ('sda_conv_wgrad3_slabs', ctypes.c_int), ('sda_conv_wgrad3_work_floats', ctypes.c_int64),
                      ('sda_conv_wgrad_emulate', ctypes.c_int), ('sda_conv_wgrad_work_floats', ctypes.c_int64)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, [ctypes.POINTER(WgradDesc)]
    return lib


@pytest.fixture(scope='module')
def cases():
    """name -> (case, float64 dW, float64 db): built once, never written."""
    out = {}
    for name in CASES:
        case = build(name, 'cpu')
        out[name] = (case, *reference(case))
    return out


def run(emu, case, slabs=0, accumulate=False, dw=None, db=None):
    cout, cin = case['cout'], case['v64'].shape[1]
    dw = torch.full((cout, cin, 3, 3), float('nan')) if dw is None else dw
    db = torch.full((cout,), float('nan')) if db is None else db
    d = wgrad_desc(case, dw, db, slabs=slabs, accumulate=accumulate)
    floats = int(emu.sda_conv_wgrad3_work_floats(ctypes.byref(d)))
    assert floats > 0, floats
    work = torch.full((floats,), float('nan'))
    d = wgrad_desc(case, dw, db, work, slabs=slabs, accumulate=accumulate)
    assert emu.sda_conv_wgrad3_emulate(ctypes.byref(d)) == 0
    return dw, db


def serves(emu, case):
    cout, cin, kh, kw = case['cout'], case['v64'].shape[1], case['kh'], case['kw']
    dw, db = torch.empty(cout, cin, kh, kw), torch.empty(cout)
    return emu.sda_conv_wgrad3_serves(ctypes.byref(wgrad_desc(case, dw, db)))


def test_serves_the_block_convolution_forms(emu, cases):
    for name, (case, _rw, _rb) in cases.items():
        assert serves(emu, case) == 1, name
    # the fourth form: plain loader with zero padding
    assert serves(emu, make_case('plain', 'cpu', cin=32, cout=32, n=2, h=8, w=8, circular=False)) == 1
    # the shapes of a Kolmogorov step's block convolutions
    for c, s in ((96, 64), (192, 32), (384, 16)):
        assert serves(emu, make_case('conv2', 'cpu', cin=c, cout=c, n=1, h=s, w=s)) == 1, (c, s)


@pytest.mark.parametrize('departure', ['stride2', 'up2', 'one_d', 'kh1', 'cx10', 'cctx', 'strided_view', 'cout48'])
def test_serves_refuses_each_single_departure(emu, departure):
    base = dict(cin=32, cout=32, n=2, h=8, w=8)
    if departure == 'stride2':
        case = make_case('head_s2', 'cpu', **base)
    elif departure == 'up2':
        case = make_case('tail_up', 'cpu', **base)
    elif departure == 'one_d':
        case = make_case('plain', 'cpu', one_d=True, **base)
    elif departure == 'kh1':
        case = make_case('plain', 'cpu', ksize=(1, 3), **base)
    elif departure == 'cx10':
        case = make_case('plain', 'cpu', **dict(base, cin=10))
    elif departure == 'cctx':
        case = make_case('head0_ctx', 'cpu', **dict(base, cin=33))           # 32 source channels + one context plane
        assert case['conv'].cx == 32 and case['conv'].cctx == 1
    elif departure == 'strided_view':
        case = make_case('plain', 'cpu', **base)                            # channel-last view of the same numbers of elements
        case['conv'].x_sx, case['conv'].x_sy, case['conv'].x_sc = 32, 32 * 8, 1
    else:
        case = make_case('plain', 'cpu', **dict(base, cout=48))
    assert serves(emu, case) == 0
    cout, cin, kh, kw = case['cout'], case['v64'].shape[1], case['kh'], case['kw']
    dw, db, work = torch.zeros(cout, cin, kh, kw), torch.zeros(cout), torch.zeros(16)
    d = wgrad_desc(case, dw, db, work)
    assert emu.sda_conv_wgrad3_work_floats(ctypes.byref(d)) == -2            # SDA_E_UNSUPPORTED
    assert emu.sda_conv_wgrad3_emulate(ctypes.byref(d)) == -2
    assert emu.sda_conv_wgrad_work_floats(ctypes.byref(d)) > 0               # ... and the general kernel takes it


@pytest.mark.parametrize('name', list(CASES))
def test_emulated_result_matches_float64(emu, cases, name):
    case, rw, rb = cases[name]
    dw, db = run(emu, case)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    print(name, 'rel err dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))


@pytest.mark.parametrize('name', list(CASES))
def test_emulated_result_is_bitwise_reproducible(emu, cases, name):
    case = cases[name][0]
    dw, db = run(emu, case)
    dw2, db2 = run(emu, case)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('name', list(CASES))
def test_forced_slab_counts_agree(emu, cases, name):
    case, rw, rb = cases[name]
    cout, cin = case['cout'], case['v64'].shape[1]
    dw0, db0 = torch.empty(cout, cin, 3, 3), torch.empty(cout)
    for slabs in (1, 2, 0):
        dw, db = run(emu, case, slabs)
        assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (slabs, rel_err(dw, rw), rel_err(db, rb))
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=1))) == 1
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=2))) == 2
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=257))) < 0


def test_ragged_row_block_and_ragged_last_slab(emu):
    # 14 rows in blocks of 12 (W + 2 = 10): the second block of every image has 2 live rows; 10 stages in 3 slabs of 4, 4, 2
    case = make_case('conv1', 'cpu', cin=32, cout=32, n=5, h=14, w=8, circular=True, seed=44)
    cout, cin = 32, 32
    d = wgrad_desc(case, torch.empty(cout, cin, 3, 3), torch.empty(cout), slabs=3)
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(d)) == 3
    rw, rb = reference(case)
    for circ in (True, False):
        case = make_case('conv1', 'cpu', cin=32, cout=32, n=5, h=14, w=8, circular=circ, seed=44)
        rw, rb = reference(case)
        dw, db = run(emu, case, slabs=3)
        assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (circ, rel_err(dw, rw), rel_err(db, rb))


def test_accumulate_adds_onto_a_prior(emu, cases):
    case = cases['wrap'][0]
    dw, db = run(emu, case)
    gen = torch.Generator().manual_seed(45)
    pw, pb = torch.randn(dw.shape, generator=gen) * 5, torch.randn(db.shape, generator=gen) * 5
    dw2, db2 = run(emu, case, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, pw + dw) and torch.equal(db2, pb + db)


def test_agrees_with_the_general_replay(emu, cases):
    case, rw, rb = cases['ln_mod']
    dw, db = run(emu, case)
    gw, gb = torch.full_like(dw, float('nan')), torch.full_like(db, float('nan'))
    d = wgrad_desc(case, gw, gb)
    work = torch.empty(int(emu.sda_conv_wgrad_work_floats(ctypes.byref(d))))
    assert emu.sda_conv_wgrad_emulate(ctypes.byref(wgrad_desc(case, gw, gb, work))) == 0
    assert rel_err(dw, gw) <= TOL and rel_err(db, gb) <= TOL


# ---------------------------------------------------------------------------------------- the switch

def test_switch_sets_and_restores():
    assert training.wgrad_route() == 'general'
    with training.parameter_gradients(wgrad='tiled'):
        assert training.enabled() and training.wgrad_route() == 'tiled'
        with training.parameter_gradients():
            assert training.wgrad_route() == 'general'
        assert training.wgrad_route() == 'tiled'
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_switch_refuses_a_bad_name():
    with pytest.raises(ValueError):
        with training.parameter_gradients(wgrad='winograd'):
            pass
    with pytest.raises(ValueError):
        training.enable(wgrad='fast')
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_switch_nests_with_mlp():
    with training.parameter_gradients(mlp=True):
        assert training.mlp_enabled() and training.wgrad_route() == 'general'
        with training.parameter_gradients(mlp=True, wgrad='tiled'):
            assert training.mlp_enabled() and training.wgrad_route() == 'tiled'
        assert training.mlp_enabled() and training.wgrad_route() == 'general'
    assert not training.mlp_enabled() and training.wgrad_route() == 'general'


def test_enable_and_disable():
    try:
        training.enable(mlp=True, wgrad='tiled')
        assert training.enabled() and training.mlp_enabled() and training.wgrad_route() == 'tiled'
    finally:
        training.disable()
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_ops_and_loop_take_the_route():
    import inspect
    from sda_amd import ops, utils
    assert inspect.signature(ops.conv_wgrad).parameters['route'].default == 'general'
    assert inspect.signature(utils.loop).parameters['wgrad'].default == 'general'
    with pytest.raises(ValueError):
        ops.conv_wgrad(None, None, None, None, False, route='other')
