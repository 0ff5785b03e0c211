"""CPU: the tiled weight-gradient kernel of the stride-2 heads and up-sampling tails (csrc/conv_wgrad3.hip, sda_conv_wgrad3x) -- its served set and the
widths at which the LDS cap ends it, its plan and host replay against float64 over the case table (tests/wgrad3x_cases.py) and a
sample of tests/fuzz/wgrad3x_fuzz.py, and the ``wgrad='tiled_ht'`` switch.

The replay in libsda_emu.so shares the planner, the staging walk and the two staging maps (the up-sampled tile; the four parity
planes), the tap offsets, the MFMA lane maps and the slab-ordered reduction with the gfx950 kernel, and refuses any LDS index outside
the image.  The device kernel is tested in test_gpu_wgrad3x.py.  The bound against float64 is the one test_wgrad3_host.py and
test_wgrad_emulator.py hold for the same arithmetic class (1e-5 of the largest element)."""
import ctypes

import pytest
import torch

from sda_amd import build as sbuild
from sda_amd import training
from sda_amd._lib import WgradDesc
from tests.util import rel_err
from tests.wgrad3x_cases import BOUNDARY, CASES, LDS_MAX, PLANS, S2, UP2, UP2_PLAIN, boundary_case, build, make, out_size, plan
from tests.wgrad_ref import make_case, reference, wgrad_desc

TOL = 1e-5
PLAN_FIELDS = ('mode', 'R', 'nrb', 'S', 'mt', 'n_ct', 'n_cit', 'q4', 'vp', 'gp', 'lds_bytes', 'per', 'slabs', 'grid')


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    for name, res in (('sda_conv_wgrad3x_emulate', ctypes.c_int), ('sda_conv_wgrad3x_serves', ctypes.c_int),
                      ('sda_conv_wgrad3x_slabs', ctypes.c_int), ('sda_conv_wgrad3x_work_floats', ctypes.c_int64),
                      ('sda_conv_wgrad3_serves', ctypes.c_int),
                      ('sda_conv_wgrad_emulate', ctypes.c_int), ('sda_conv_wgrad_work_floats', ctypes.c_int64)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, [ctypes.POINTER(WgradDesc)]
    lib.sda_conv_wgrad3x_plan.restype = ctypes.c_int
    lib.sda_conv_wgrad3x_plan.argtypes = [ctypes.POINTER(WgradDesc), ctypes.POINTER(ctypes.c_int)]
    return lib


@pytest.fixture(scope='module')
def cases():
    """name -> (case, float64 dW, float64 db): built once, never written."""
    out = {}
    for name in CASES:
        case = build(name, 'cpu')
        out[name] = (case, *reference(case))
    return out


def run(emu, case, slabs=0, accumulate=False, dw=None, db=None, with_db=True):
    cout, cin = case['cout'], case['v64'].shape[1]
    dw = torch.full((cout, cin, 3, 3), float('nan')) if dw is None else dw
    db = torch.full((cout,), float('nan')) if db is None else db
    dbp = db if with_db else None
    d = wgrad_desc(case, dw, dbp, slabs=slabs, accumulate=accumulate)
    floats = int(emu.sda_conv_wgrad3x_work_floats(ctypes.byref(d)))
    assert floats > 0, floats
    work = torch.full((floats,), float('nan'))
    d = wgrad_desc(case, dw, dbp, work, slabs=slabs, accumulate=accumulate)
    assert emu.sda_conv_wgrad3x_emulate(ctypes.byref(d)) == 0
    return dw, db


def planned(name, slabs=0):
    cfg = CASES[name]
    return plan(cfg['kind'], cfg['cin'], cfg['cout'], cfg['n'], cfg['h'], cfg['w'], slabs)


def empty_grads(case):
    return torch.empty(case['cout'], case['v64'].shape[1], case['kh'], case['kw']), torch.empty(case['cout'])


def serves(emu, case):
    return emu.sda_conv_wgrad3x_serves(ctypes.byref(wgrad_desc(case, *empty_grads(case))))


def library_plan(emu, case, slabs=0):
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    assert emu.sda_conv_wgrad3x_plan(ctypes.byref(wgrad_desc(case, *empty_grads(case), slabs=slabs)), out) == 0
    return dict(zip(PLAN_FIELDS, out))


def test_serves_the_heads_and_tails(emu, cases):
    for name, (case, _rw, _rb) in cases.items():
        assert serves(emu, case) == 1, name
        assert emu.sda_conv_wgrad3_serves(ctypes.byref(wgrad_desc(case, *empty_grads(case)))) == 0, name      # (the other kernel's set is apart)
    # the four head and tail shapes of a Kolmogorov step
    for kind, cin, cout, s in ((S2, 96, 192, 64), (S2, 192, 384, 32), (UP2, 384, 192, 16), (UP2, 192, 96, 32)):
        assert serves(emu, make_case(kind, 'cpu', cin=cin, cout=cout, n=1, h=s, w=s)) == 1, (kind, cin, cout, s)


DEPARTURES = ['stride1', 'up2_stride2', 'one_d', 'cx10', 'cctx', 'strided_view', 'cout48', 'odd_hs', 'modulation']
# (an odd source height is a departure of the stride-2 geometry only: the up-sampling one serves it, see 'up_ragged')
DEPARTURE_PAIRS = [(kind, dep) for kind in (UP2, S2) for dep in DEPARTURES if (kind, dep) != (UP2, 'odd_hs')]


@pytest.mark.parametrize('kind,departure', DEPARTURE_PAIRS)
def test_serves_refuses_each_single_departure(emu, kind, departure):
    base = dict(cin=32, cout=32, n=2, h=8, w=8)
    keep = []
    case = make_case(kind, 'cpu', **base)
    assert serves(emu, case) == 1
    if departure == 'stride1':                                               # (the other tiled kernel's layer)
        case = make_case('plain', 'cpu', **base)
    elif departure == 'up2_stride2':                                         # 8 x 8 up-sampled to 16 x 16, then stride 2: 8 x 8
        case['conv'].stride_h = case['conv'].stride_w = case['conv'].up_h = case['conv'].up_w = 2
        case['conv'].ho = case['conv'].wo = 8
        case['g'] = torch.randn(2, 32, 8, 8)
    elif departure == 'one_d':
        case = make_case(kind, 'cpu', one_d=True, **base)
    elif departure == 'cx10':
        case = make_case(kind, 'cpu', **dict(base, cin=10))
    elif departure == 'cctx':                                                # 32 source channels + one context plane
        ctx = torch.randn(8 * 8)
        keep.append(ctx)
        case['conv'].ctx, case['conv'].cctx, case['conv'].ctx_sn = ctx.data_ptr(), 1, 0
        case['v64'] = torch.cat([case['v64'], torch.zeros_like(case['v64'][:, :1])], dim=1)       # (33 input channels: shapes only)
    elif departure == 'strided_view':                                        # channel-last view of the same number of elements
        case['conv'].x_sx, case['conv'].x_sy, case['conv'].x_sc = 32, 32 * 8, 1
    elif departure == 'cout48':
        case = make_case(kind, 'cpu', **dict(base, cout=48))
    elif departure == 'odd_hs':
        case = make_case(kind, 'cpu', **dict(base, h=7))
    else:                                                                    # a modulation row in front of the loader
        mod = torch.randn(2, 32)
        keep.append(mod)
        case['conv'].mod, case['conv'].mod_sn = mod.data_ptr(), 32
    assert serves(emu, case) == 0
    dw, db = empty_grads(case)
    d = wgrad_desc(case, dw.zero_(), db.zero_(), torch.zeros(16))
    assert emu.sda_conv_wgrad3x_work_floats(ctypes.byref(d)) == -2           # SDA_E_UNSUPPORTED
    assert emu.sda_conv_wgrad3x_emulate(ctypes.byref(d)) == -2
    assert emu.sda_conv_wgrad_work_floats(ctypes.byref(d)) > 0               # ... and the general kernel still plans it


@pytest.mark.parametrize('name', list(CASES))
def test_plan_is_the_expected_one(emu, cases, name):
    """The table's hand-written plan, the plan worked out in Python and the library's planner agree, field by field."""
    case, want, got = cases[name][0], PLANS[name], planned(name)
    assert {k: got[k] for k in want} == want
    cout, cin = case['cout'], case['v64'].shape[1]
    d = wgrad_desc(case, *empty_grads(case))
    assert emu.sda_conv_wgrad3x_slabs(ctypes.byref(d)) == want['slabs']
    assert emu.sda_conv_wgrad3x_work_floats(ctypes.byref(d)) == want['slabs'] * cout * (cin * 9 + 1)
    lib = library_plan(emu, case)
    assert lib['mode'] == (1 if CASES[name]['kind'] == S2 else 0)
    assert {k: lib[k] for k in got if k in lib} == {k: got[k] for k in got if k in lib}
    assert lib['grid'] == got['n_ct'] * got['n_cit'] * got['slabs']
    assert got['lds_bytes'] <= LDS_MAX and got['vp'] % 32 == 2 and got['gp'] % 32 == 2


def test_table_moves_every_plan_dimension():
    for geom in ('up_', 's2_'):
        plans = [p for name, p in PLANS.items() if name.startswith(geom)]
        names = [name for name in CASES if name.startswith(geom)]
        assert {p['mt'] for p in plans if p['n_ct'] > 1 and p['n_cit'] > 1} == {1, 2, 3}
        assert any(p['R'] == 1 and p['nrb'] > 1 for p in plans) and any(p['R'] > 1 and p['nrb'] > 1 for p in plans)
        assert any(p['q4_rounds'] for p in plans) and any(not p['q4_rounds'] for p in plans)
        assert any(planned(name)['per'] > 1 for name in names)
        assert {CASES[name]['circular'] for name in names} == {True, False}
        assert any(CASES[name]['h'] != CASES[name]['w'] for name in names)
        # a ragged last row block
        assert any(out_size(CASES[n]['kind'], CASES[n]['h'], CASES[n]['w'])[0] % PLANS[n]['R'] for n in names)
    assert any(CASES[name]['kind'] == UP2_PLAIN for name in CASES)


@pytest.mark.parametrize('name', list(CASES))
def test_emulated_result_matches_float64(emu, cases, name):
    case, rw, rb = cases[name]
    dw, db = run(emu, case)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    print(name, 'rel err dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))
    dw2, db2 = run(emu, case)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('name', ['up_wrap', 'up_zero', 'up_plain', 'up_ct_mt3', 'up_row1', 's2_wrap', 's2_zero', 's2_ct_mt2', 's2_q4_tail',
                                  's2_one_pixel'])
def test_agrees_with_the_general_replay(emu, cases, name):
    case, rw, rb = cases[name]
    dw, db = run(emu, case)
    gw, gb = torch.full_like(dw, float('nan')), torch.full_like(db, float('nan'))
    d = wgrad_desc(case, gw, gb)
    work = torch.empty(int(emu.sda_conv_wgrad_work_floats(ctypes.byref(d))))
    assert emu.sda_conv_wgrad_emulate(ctypes.byref(wgrad_desc(case, gw, gb, work))) == 0
    assert rel_err(dw, gw) <= TOL and rel_err(db, gb) <= TOL, (rel_err(dw, gw), rel_err(db, gb))


@pytest.mark.parametrize('name', ['up_ragged', 'up_q4_tail', 'up_workload_16', 's2_ragged_zero', 's2_workload_16', 's2_planner_per2'])
def test_forced_slab_counts_agree(emu, cases, name):
    case, rw, rb = cases[name]
    dw0, db0 = empty_grads(case)
    for slabs in (1, 2, 3):
        dw, db = run(emu, case, slabs)
        assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (slabs, rel_err(dw, rw), rel_err(db, rb))
        want = planned(name, slabs)
        assert want['slabs'] <= slabs
        assert emu.sda_conv_wgrad3x_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=slabs))) == want['slabs']
        assert library_plan(emu, case, slabs)['per'] == want['per']
    assert emu.sda_conv_wgrad3x_slabs(ctypes.byref(wgrad_desc(case, dw0, db0, slabs=257))) < 0


@pytest.mark.parametrize('name', ['up_wrap', 's2_zero'])
def test_accumulate_adds_onto_a_prior(emu, cases, name):
    case = cases[name][0]
    dw, db = run(emu, case)
    gen = torch.Generator().manual_seed(45)
    pw, pb = torch.randn(dw.shape, generator=gen) * 5, torch.randn(db.shape, generator=gen) * 5
    dw2, db2 = run(emu, case, accumulate=True, dw=pw.clone(), db=pb.clone())
    assert torch.equal(dw2, pw + dw) and torch.equal(db2, pb + db)


@pytest.mark.parametrize('name', ['up_ct_mt2', 's2_ct_mt3'])
def test_no_bias_gradient_leaves_db_alone(emu, cases, name):
    case, rw, _rb = cases[name]
    dw, db = run(emu, case, with_db=False)
    assert rel_err(dw, rw) <= TOL and torch.isnan(db).all()


# ---------------------------------------------------------------------------------------- the served width

def test_lds_cap_by_hand():
    """The boundary widths from the pitches alone, at one row per stage (q4 = wo + 2 rounded up to 4): the up-sampled image spans
    q4 + 2 (wo + 2) + 2 floats a channel, the four parity planes 3 x 2 (wo + 2) + q4 + (wo + 2) + 1; 32 input and 32 mt cotangent
    channels at 2 (mod 32) pitches."""
    for (kind, cout), w in BOUNDARY.items():
        h, step = (1, 1) if kind == UP2 else (2, 2)
        p = plan(kind, 32, cout, 1, h, w)
        assert p['R'] == 1 and p['lds_bytes'] <= LDS_MAX < plan(kind, 32, cout, 1, h, w + step)['lds_bytes'], (kind, cout)
    assert plan(UP2, 32, 32, 1, 1, 153)['lds_bytes'] == 4 * 32 * (930 + 322)        # wo = 306: 160256 of 163840 bytes
    assert plan(S2, 32, 32, 1, 2, 268)['lds_bytes'] == 4 * 32 * (1090 + 162)        # wo = 134: 7 x 136 + 136 + 1 = 1089 -> 1090
    assert plan(S2, 32, 96, 1, 2, 212)['lds_bytes'] == 4 * (32 * 866 + 96 * 130)    # wo = 106: 7 x 108 + 108 + 1 = 865 -> 866
    # the workload: the two heads take one workgroup's worth of a CU's LDS, the two tails under half of it
    assert plan(S2, 96, 192, 32, 64, 64)['lds_bytes'] == 123904 and plan(S2, 192, 384, 32, 32, 32)['lds_bytes'] == 128000
    assert plan(UP2, 384, 192, 32, 16, 16)['lds_bytes'] == 74752 and plan(UP2, 192, 96, 32, 32, 32)['lds_bytes'] == 66560


@pytest.mark.parametrize('kind,cout', list(BOUNDARY))
def test_served_width_boundary(emu, kind, cout):
    wmax = BOUNDARY[(kind, cout)]
    h, step = (1, 1) if kind == UP2 else (2, 2)
    probe = lambda w: make_case(kind, 'cpu', cin=32, cout=cout, n=1, h=h, w=w)
    unserved = [w for w in range(step, wmax + 1, step) if serves(emu, probe(w)) != 1]
    assert not unserved, unserved
    assert serves(emu, probe(wmax + step)) == 0
    over = boundary_case(kind, cout, 'cpu', over=1)
    assert serves(emu, over) == 0
    d = wgrad_desc(over, *empty_grads(over))
    assert emu.sda_conv_wgrad3x_work_floats(ctypes.byref(d)) == -2
    assert emu.sda_conv_wgrad_work_floats(ctypes.byref(d)) > 0                   # ... and the general kernel takes the launch
    case = boundary_case(kind, cout, 'cpu')
    assert serves(emu, case) == 1
    assert library_plan(emu, case)['lds_bytes'] == plan(kind, 32, cout, 1, h, wmax)['lds_bytes']
    rw, rb = reference(case)
    dw, db = run(emu, case)
    print(kind, cout, wmax, 'rel err dw', rel_err(dw, rw), 'db', rel_err(db, rb))
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL, (rel_err(dw, rw), rel_err(db, rb))


# ---------------------------------------------------------------------------------------- the fuzz sample

def load_wgrad3x_fuzz():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        'wgrad3x_fuzz', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz', 'wgrad3x_fuzz.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


FUZZ_SEED, FUZZ_CASES = 11, 60        # (tests/test_gpu_wgrad3x.py runs the same draws on the device)


def fuzz_corners(cfg):
    """The corners of the plan a draw reaches (the sample is there for them), each tagged with its geometry."""
    p = cfg['plan']
    geom = 's2' if cfg['kind'] == S2 else 'up2'
    ho, wo = out_size(cfg['kind'], cfg['h'], cfg['w'])
    tags = {'n_ct' if p['n_ct'] > 1 else '', 'n_cit' if p['n_cit'] > 1 else '', 'row1' if p['R'] == 1 and wo + 2 > 64 else '',
            'q4' if p['q4_rounds'] else '', 'ragged' if ho % p['R'] else '', 'one_pixel' if min(cfg['h'], cfg['w']) <= (2 if geom == 's2' else 1) else '',
            'accumulate' if cfg['accumulate'] else '', 'no_db' if not cfg['with_db'] else '',
            'forced_slabs' if cfg['slabs'] else 'planner_slabs', 'circular' if cfg['circ'] else 'zeros', f"mt{p['mt']}"}
    out = {f'{geom}:{t}' for t in tags if t}
    if p['per'] > 1 and not cfg['slabs']:
        out.add('planner_per')
    out.add(cfg['kind'])
    return out


FUZZ_CORNERS = {f'{g}:{t}' for g in ('up2', 's2') for t in ('n_ct', 'n_cit', 'row1', 'q4', 'ragged', 'one_pixel', 'accumulate', 'no_db',
                                                             'forced_slabs', 'planner_slabs', 'circular', 'zeros', 'mt1', 'mt2', 'mt3')}
FUZZ_CORNERS |= {'planner_per', UP2, UP2_PLAIN, S2}


def test_wgrad3x_fuzz_sample():
    """A bounded sample of tests/fuzz/wgrad3x_fuzz.py on the replay: random served layers over both geometries, every cout tile, tile
    count, planner threshold, padding mode, slab count, accumulation and a missing bias gradient.  No draw is skipped; a draw the
    planner refuses fails."""
    import random
    fuzz = load_wgrad3x_fuzz()
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
    with training.parameter_gradients(wgrad='tiled_ht'):
        assert training.enabled() and training.wgrad_route() == 'tiled_ht'
        with training.parameter_gradients(wgrad='tiled'):
            assert training.wgrad_route() == 'tiled'
            with training.parameter_gradients():
                assert training.wgrad_route() == 'general'
            assert training.wgrad_route() == 'tiled'
        assert training.wgrad_route() == 'tiled_ht'
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_switch_nests_with_mlp():
    with training.parameter_gradients(mlp=True):
        assert training.mlp_enabled() and training.wgrad_route() == 'general'
        with training.parameter_gradients(mlp=True, wgrad='tiled_ht'):
            assert training.mlp_enabled() and training.wgrad_route() == 'tiled_ht'
        assert training.mlp_enabled() and training.wgrad_route() == 'general'
    assert not training.mlp_enabled() and training.wgrad_route() == 'general'


def test_enable_and_disable():
    try:
        training.enable(mlp=True, wgrad='tiled_ht')
        assert training.enabled() and training.mlp_enabled() and training.wgrad_route() == 'tiled_ht'
    finally:
        training.disable()
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_route_names_and_refusals():
    from sda_amd import ops
    assert training.WGRAD_ROUTES == ops.WGRAD_ROUTES == ('general', 'tiled', 'tiled_ht')
    for bad in ('tiled_h', 'ht', 'winograd'):
        with pytest.raises(ValueError, match="'general', 'tiled' or 'tiled_ht'"):
            training.enable(wgrad=bad)
        with pytest.raises(ValueError, match="'general', 'tiled' or 'tiled_ht'"):
            ops.conv_wgrad(None, None, None, None, False, route=bad)
    assert not training.enabled() and training.wgrad_route() == 'general'


def test_ops_and_loop_take_the_route():
    """``ops.conv_wgrad(route='tiled_ht')`` gets past the route check (the next check, a device tensor, stops it here: no GPU) and
    ``utils.loop(wgrad='tiled_ht')`` switches the route on for its training steps."""
    import inspect
    from sda_amd import ops, utils
    assert inspect.signature(ops.conv_wgrad).parameters['route'].default == 'general'
    assert inspect.signature(utils.loop).parameters['wgrad'].default == 'general'
    case = build('s2_wrap', 'cpu')
    dw, db = empty_grads(case)
    with pytest.raises(Exception) as err:
        ops.conv_wgrad(case['conv'], case['g'], dw, db, False, route='tiled_ht')
    assert not isinstance(err.value, ValueError), err.value

    seen = []

    class Sde(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.ones(()))

        def loss(self, x):
            seen.append(training.wgrad_route())
            return (self.p * x).square().mean()

    data = [(torch.ones(2), {}) for _ in range(4)]
    next(utils.loop(Sde(), data, data, epochs=1, batch_size=2, wgrad='tiled_ht'))
    assert seen and seen[0] == 'tiled_ht' and training.wgrad_route() == 'general'
