"""CPU: the tiled 3 x 3 weight-gradient kernel (csrc/conv_wgrad3.hip) -- its served set and the width at which the LDS cap ends it,
its plan and host replay against float64 over the case table (tests/wgrad3_cases.py) and a sample of tests/fuzz/wgrad3_fuzz.py, and the
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
from tests.wgrad3_cases import BOUNDARY, CASES, LDS_MAX, PLANS, boundary_case, build, plan
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


def planned(name, slabs=0):
    cfg = CASES[name]
    return plan(cfg['cin'], cfg['cout'], cfg['n'], cfg['h'], cfg['w'], slabs)


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
def test_plan_is_the_expected_one(emu, cases, name):
    """The table's hand-written plan, the plan worked out in Python and what the library's planning entries expose agree."""
    case, want, got = cases[name][0], PLANS[name], planned(name)
    assert {k: got[k] for k in want} == want
    cout, cin = case['cout'], case['v64'].shape[1]
    d = wgrad_desc(case, torch.empty(cout, cin, 3, 3), torch.empty(cout))
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(d)) == want['slabs']
    assert emu.sda_conv_wgrad3_work_floats(ctypes.byref(d)) == want['slabs'] * cout * (cin * 9 + 1)
    assert got['lds_bytes'] <= LDS_MAX


def test_table_moves_every_plan_dimension():
    plans = PLANS.values()
    assert {p['mt'] for p in plans if p['n_ct'] > 1} == {1, 2, 3}
    assert any(p['n_ct'] > 1 and p['n_cit'] > 1 for p in plans)
    assert any(p['R'] == 1 and p['nrb'] > 1 for p in plans) and any(p['R'] > 1 and p['nrb'] > 1 for p in plans)
    assert any(p['q4_rounds'] for p in plans)
    assert any(planned(name)['per'] > 1 for name in CASES)


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
    two = min(2, planned(name)['S'])                                         # (no empty slab: one stage makes one slab)
    assert planned(name, 2)['slabs'] == two
    assert emu.sda_conv_wgrad3_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=2))) == two
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


# ---------------------------------------------------------------------------------------- the served width

def test_lds_cap_by_hand():
    """The boundary widths from the pitches alone: h = 2 and W + 2 > 64 give one row per stage, q4 = W + 2 rounded up to 4, the
    input tile spans q4 + 2 (W + 2) + 2 floats a channel; 32 input and 32 mt cotangent channels at 2 (mod 32) pitches."""
    for cout, w in BOUNDARY.items():
        assert plan(32, cout, 1, 2, w)['lds_bytes'] <= LDS_MAX < plan(32, cout, 1, 2, w + 1)['lds_bytes'], cout
    assert plan(32, 32, 1, 2, 306)['lds_bytes'] == 4 * 32 * (930 + 322)         # 160256 of 163840 bytes
    assert BOUNDARY[32] + 2 < 4096                                              # (the W + 2 > 4096 refusal is unreachable behind it)


@pytest.mark.parametrize('cout', list(BOUNDARY))
def test_served_width_boundary(emu, cout):
    wmax = BOUNDARY[cout]

    probe = lambda w: make_case('plain', 'cpu', cin=32, cout=cout, n=1, h=2, w=w)
    unserved = [w for w in range(1, wmax + 1) if serves(emu, probe(w)) != 1]
    assert not unserved, unserved
    assert serves(emu, probe(wmax + 1)) == 0
    over = boundary_case(cout, 'cpu', over=1)
    assert serves(emu, over) == 0
    d = wgrad_desc(over, torch.empty(cout, 32, 3, 3), torch.empty(cout))
    assert emu.sda_conv_wgrad3_work_floats(ctypes.byref(d)) == -2
    assert emu.sda_conv_wgrad_work_floats(ctypes.byref(d)) > 0                   # ... and the general kernel takes the launch
    case = boundary_case(cout, 'cpu')
    assert serves(emu, case) == 1
    rw, rb = reference(case)
    dw, db = run(emu, case)
    print(cout, wmax, 'rel err dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))


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


# ---------------------------------------------------------------------------------------- the fuzz sample

def load_wgrad3_fuzz():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        'wgrad3_fuzz', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz', 'wgrad3_fuzz.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


FUZZ_SEED, FUZZ_CASES = 7, 40         # (tests/test_gpu_wgrad3.py runs the same draws on the device)


def fuzz_corners(cfg):
    """The corners of the plan a draw reaches (the sample is there for them)."""
    p = cfg['plan']
    return {'n_ct' if p['n_ct'] > 1 else '', 'row1' if p['R'] == 1 and cfg['w'] + 2 > 64 else '', 'q4' if p['q4_rounds'] else '',
            'accumulate' if cfg['accumulate'] else '', 'per' if p['per'] > 1 else '', 'no_db' if not cfg['with_db'] else '',
            'forced_slabs' if cfg['slabs'] else 'planner_slabs', 'circular' if cfg['circ'] else 'zeros', cfg['kind'], cfg['act'] or ''}


FUZZ_CORNERS = {'n_ct', 'row1', 'q4', 'accumulate', 'per', 'no_db', 'forced_slabs', 'planner_slabs', 'circular', 'zeros', 'plain', 'conv1',
                'conv1_shared', 'conv2', 'SiLU', 'ReLU', 'ELU', 'GELU', 'SELU'}


def test_wgrad3_fuzz_sample():
    """A bounded sample of tests/fuzz/wgrad3_fuzz.py on the replay: random served layers over every loader, cout tile, tile count,
    planner threshold, padding mode, slab count, accumulation and a missing bias gradient.  No case is skipped; a draw the planner
    refuses fails."""
    import random
    fuzz = load_wgrad3_fuzz()
    backend = fuzz.emulator()
    rng = random.Random(FUZZ_SEED)
    bad, seen = [], set()
    for i in range(FUZZ_CASES):
        cfg, msg = fuzz.one_case(rng, backend, i)
        seen |= fuzz_corners(cfg)
        if msg:
            bad.append((i, msg, cfg))
    assert not bad, '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)
    # the sample reaches every corner it is there for
    assert seen >= FUZZ_CORNERS, FUZZ_CORNERS - seen


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
