"""CPU: the weight-gradient tile algorithm (csrc/conv_wgrad.hip) replayed on the host against float64 torch.autograd.

The emulator shares the planner, the column / position decoders, the loader (source view, context channels, modulation +
LayerNorm, activation, nearest up-sample, stride, circular / zero padding) and the slab-ordered reduction with the gfx950
kernel, so these tests pin its index arithmetic without a GPU.  The device kernel is tested in test_gpu_training.py."""
import ctypes

import pytest
import torch

from sda_amd import build as sbuild
from sda_amd._lib import WgradDesc
from tests.wgrad_ref import make_case, reference, wgrad_desc, work_floats
from tests.util import rel_err


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_conv_wgrad_emulate.restype = ctypes.c_int
    lib.sda_conv_wgrad_emulate.argtypes = [ctypes.POINTER(WgradDesc)]
    lib.sda_conv_wgrad_work_floats.restype = ctypes.c_int64
    lib.sda_conv_wgrad_work_floats.argtypes = [ctypes.POINTER(WgradDesc)]
    lib.sda_conv_wgrad_slabs.restype = ctypes.c_int
    lib.sda_conv_wgrad_slabs.argtypes = [ctypes.POINTER(WgradDesc)]
    return lib


def run(emu, case, slabs=0, accumulate=False, dw=None, db=None):
    cout, cin, kh, kw = case['cout'], case['v64'].shape[1], case['kh'], case['kw']
    dw = torch.full((cout, cin, kh, kw), float('nan')) if dw is None else dw
    db = torch.full((cout,), float('nan')) if db is None else db
    d = wgrad_desc(case, dw, db, slabs=slabs, accumulate=accumulate)
    work = torch.full((work_floats(emu, d),), float('nan'))
    d = wgrad_desc(case, dw, db, work, slabs=slabs, accumulate=accumulate)
    assert emu.sda_conv_wgrad_emulate(ctypes.byref(d)) == 0
    return dw, db


def check(emu, case, slabs=0, tol=1e-5):
    dw, db = run(emu, case, slabs)
    rw, rb = reference(case)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert rel_err(dw, rw) <= tol, rel_err(dw, rw)
    assert rel_err(db, rb) <= tol, rel_err(db, rb)


@pytest.mark.parametrize('kind', ['plain', 'conv1', 'conv1_shared', 'conv2', 'tail_up', 'head_s2', 'head0_ctx', 'head0_window'])
@pytest.mark.parametrize('circular', [True, False])
def test_wgrad_variants(emu, kind, circular):
    check(emu, make_case(kind, 'cpu', cin=9, cout=12, n=2, h=6, w=8, circular=circular, seed=1))


@pytest.mark.parametrize('act', ['SiLU', 'ReLU', 'ELU', 'GELU', 'SELU'])
def test_wgrad_conv2_activations(emu, act):
    check(emu, make_case('conv2', 'cpu', cin=6, cout=5, n=1, h=5, w=5, act=act, seed=2))


def test_wgrad_ten_channel_tail(emu):
    # the level-0 tail: C -> 10 output channels (Kolmogorov: window 5 x 2 channels)
    check(emu, make_case('tail10', 'cpu', cin=16, cout=10, n=3, h=8, w=8, seed=3))


def test_wgrad_ten_channel_head(emu):
    # the level-0 head reading 10 channels + the forcing plane
    check(emu, make_case('head0_ctx', 'cpu', cin=11, cout=16, n=2, h=8, w=8, seed=4))


@pytest.mark.parametrize('kind', ['conv1', 'head_s2', 'tail_up'])
def test_wgrad_odd_sizes(emu, kind):
    # odd spatial sizes: zero padding for the stride-2 head (its circular VJP needs even sizes in the engine), wrap elsewhere
    check(emu, make_case(kind, 'cpu', cin=7, cout=33, n=3, h=7, w=5, circular=kind != 'head_s2', seed=5))


@pytest.mark.parametrize('kind', ['plain', 'conv1', 'conv2', 'tail_up', 'head_s2'])
@pytest.mark.parametrize('circular', [True, False])
def test_wgrad_1d(emu, kind, circular):
    check(emu, make_case(kind, 'cpu', cin=6, cout=40, n=3, w=12, one_d=True, circular=circular, seed=6))


@pytest.mark.parametrize('slabs', [0, 1, 2, 3, 7, 64])
def test_wgrad_slab_counts(emu, slabs):
    case = make_case('conv1', 'cpu', cin=10, cout=70, n=4, h=8, w=8, seed=7)
    check(emu, case, slabs=slabs)


def test_wgrad_slab_plan(emu):
    case = make_case('conv2', 'cpu', cin=8, cout=8, n=2, h=8, w=8)
    dw, db = torch.empty(8, 8, 3, 3), torch.empty(8)
    for want, got in ((1, 1), (2, 2), (3, 2), (5, 4)):   # 128 positions = 4 stages of 32, equal whole-stage slabs
        assert emu.sda_conv_wgrad_slabs(ctypes.byref(wgrad_desc(case, dw, db, slabs=want))) == got
    assert emu.sda_conv_wgrad_slabs(ctypes.byref(wgrad_desc(case, dw, db, slabs=65))) < 0


def test_wgrad_accumulate(emu):
    case = make_case('conv1', 'cpu', cin=8, cout=8, n=2, h=6, w=6, seed=8)
    dw, db = run(emu, case)
    dw2, db2 = run(emu, case, accumulate=True, dw=dw.clone(), db=db.clone())
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


def test_wgrad_without_bias(emu):
    case = make_case('plain', 'cpu', cin=4, cout=4, n=1, h=4, w=4)
    dw = torch.empty(4, 4, 3, 3)
    d = wgrad_desc(case, dw, None)
    work = torch.empty(work_floats(emu, d))
    assert emu.sda_conv_wgrad_emulate(ctypes.byref(wgrad_desc(case, dw, None, work))) == 0
    assert rel_err(dw, reference(case)[0]) <= 1e-5


def load_wgrad_fuzz():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        'wgrad_fuzz', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz', 'wgrad_fuzz.py'))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


FUZZ_SEED, FUZZ_CASES = 31, 60        # (tests/test_gpu_training.py runs the same draws on the device)


def test_wgrad_fuzz_sample():
    """A bounded sample of tests/fuzz/wgrad_fuzz.py on the emulator: random descriptors over the source views (planar, channel-last,
    window view with an image offset), shared / per-image context, every loader mode, kernel sizes 1..7 with kh != kw, explicit
    padding, ragged cout tiles, slab counts, accumulation and a missing bias gradient.  No case is skipped."""
    import random
    fuzz = load_wgrad_fuzz()
    backend = fuzz.emulator()
    rng = random.Random(FUZZ_SEED)
    bad, seen = [], set()
    for i in range(FUZZ_CASES):
        cfg, msg = fuzz.one_case(rng, backend, i)
        seen |= {cfg['mode'], 'window_off' if cfg['window'] and cfg['lo'] else '', 'chan_last' if cfg['chan_last'] else '',
                 'ctx_per_image' if cfg['ctx_per_image'] else '', 'pad' if cfg['pad'] else '', 'mt4_ragged' if cfg['cout'] in (97, 100, 130) else '',
                 'khkw' if cfg['kh'] != cfg['kw'] and not cfg['one_d'] else '', 'cx1' if cfg['cx'] == 1 else ''}
        if msg:
            bad.append((i, msg, cfg))
    assert not bad, '\n'.join(f'case {i}: {m}\n    {c}' for i, m, c in bad)
    # the sample reaches every corner it is there for
    assert seen >= set(fuzz.MODES) | {'window_off', 'chan_last', 'ctx_per_image', 'pad', 'mt4_ragged', 'khkw', 'cx1'}, seen
