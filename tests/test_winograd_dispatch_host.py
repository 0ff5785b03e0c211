"""CPU: which instantiation the Winograd kernel (csrc/conv_wino4.hip: wino4_pick) and the f16x2 kernel (csrc/conv_h2.hip: h2_pick) launch.

tests/golden/wino4_dispatch.json and h2_dispatch.json were recorded from the launch ladders the two files had before the pick functions
existed: a host build of that code which noted, in place of launching, the kernel's template arguments, the launch grid, the dynamic
LDS, the planned geometry and the return code.  The pick functions, called through libsda_emu.so with the environment switches and the
CU count as arguments, must give the same answer on every case, name table rows only, and the cases must reach every row of the tables."""
import ctypes

import pytest

from sda_amd import build as sbuild
from sda_amd._lib import ConvDesc
from tests.util import load_pick_dispatch, pick_dispatch_desc

KERNELS = {'wino4': ('sda_wino4_pick', 'sda_wino4_variants', 7, 32), 'h2': ('sda_conv_h2_pick', 'sda_conv_h2_variants', 3, 16)}


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(sbuild.build_emu())
    lib.sda_wino4_pick.argtypes = [ctypes.POINTER(ConvDesc)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    lib.sda_conv_h2_pick.argtypes = [ctypes.POINTER(ConvDesc), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    for name in ('sda_wino4_variants', 'sda_conv_h2_variants'):
        getattr(lib, name).argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


@pytest.fixture(scope='module', params=sorted(KERNELS))
def kernel(request):
    cases, out_fields = load_pick_dispatch(request.param + '_dispatch')
    return KERNELS[request.param] + (cases, len(out_fields))


def variants(emu, name, width):
    fn = getattr(emu, name)
    n = fn(None, 0)
    buf = (ctypes.c_int * (width * n))()
    assert fn(buf, n) == n
    return [tuple(buf[width * i:width * i + width]) for i in range(n)]


def pick(emu, name, c, nout):
    out = (ctypes.c_int * nout)()
    d = pick_dispatch_desc(c)
    rc = getattr(emu, name)(ctypes.byref(d) if d is not None else None, *c['switches'], c['cus'], out)
    return rc, tuple(out)


def test_pick_matches_the_recorded_dispatch(emu, kernel):
    pick_fn, _, _, _, cases, nout = kernel
    assert len(cases) > 300
    for c in cases:
        rc, out = pick(emu, pick_fn, c, nout)
        assert rc == c['rc'], c
        if rc == 0:
            assert out == c['out'], c


def test_the_cases_reach_every_variant_and_name_no_other(emu, kernel):
    _, variants_fn, width, nrows, cases, _ = kernel
    table = variants(emu, variants_fn, width)
    assert len(table) == len(set(table)) == nrows                        # every instantiation the ladder reached: none was dead
    picked = {c['out'][:width] for c in cases if c['rc'] == 0}
    assert picked <= set(table), picked - set(table)
    # ... and every row without any switch (what test_wino4_every_variant / test_h2_every_variant run on the device)
    plain = {c['out'][:width] for c in cases if c['rc'] == 0 and all(c['switches']) and c['cus'] == 256}
    assert plain == set(table), set(table) - plain


def test_every_wino4_switch_decides_some_recorded_answer(emu):
    """A case recorded with one switch off pins that switch only if the answer with it on is another one: `enabled` a served launch that
    is then refused, `epi` a helper-fed launch (EPM 1 -> 2, and the 96-cout up-sampled tail ZP 1 -> 0), `zp` an up-sampled tail at both
    tiles (ZP 1 -> 0), `walk` the tile-walk digits."""
    cases, out_fields = load_pick_dispatch('wino4_dispatch')
    named = lambda out: dict(zip(out_fields, out))
    decided = {k: [] for k in range(4)}
    for c in cases:
        if sum(c['switches']) == 3 and c['cus'] == 256:
            k = c['switches'].index(0)
            rc_on, out_on = pick(emu, 'sda_wino4_pick', dict(c, switches=(1, 1, 1, 1)), len(out_fields))
            if (rc_on, out_on if rc_on == 0 else ()) != (c['rc'], c['out']):
                decided[k].append((rc_on, named(out_on) if rc_on == 0 else None, c['rc'], c['named']))
    assert all(decided.values()), {k: len(v) for k, v in decided.items()}
    assert any(on == 0 and off == -2 for on, _, off, _ in decided[0])                                       # enabled
    epi = [(a, b) for on, a, off, b in decided[1] if on == 0 and off == 0]
    assert any(a['epm'] == 1 and b['epm'] == 2 and a['zp'] == b['zp'] == 0 for a, b in epi)                 # epi: the full kernels
    assert {(a['ln'], a['silu']) for a, b in epi if a['epm'] == 1 and a['zp'] == 0} == {(0, 0), (0, 1), (1, 0)}     # ... of all three loaders
    assert any(a['zp'] == 1 and b['zp'] == 0 and a['mf'] == 3 for a, b in epi)                              # ... and the 96-cout tail
    zp = [(a, b) for on, a, off, b in decided[2] if on == 0 and off == 0]
    assert {a['mf'] for a, b in zp if a['zp'] == 1 and b['zp'] == 0} == {2, 3}                              # zp: both tiles
    assert any(a['walk'] == 1 and b['walk'] == 0 for on, a, off, b in decided[3] if on == 0 and off == 0)  # walk


def test_h2_refusals_are_recorded_at_served_geometry():
    """Each loader / epilogue refusal of h2_ok has a case it alone refuses: 16 x 16 (32 x 32 where parity planes are sampled), 32 channels,
    64 or 96 couts, no other descriptor field off."""
    cases, _ = load_pick_dispatch('h2_dispatch')
    ts = lambda c: 32 if c['pool'] == 2 or c['stride'] == 2 else 16
    alone =[c for c in cases if c['rc'] == -2 and c['extra'] == {} and c['cx'] % 32 == 0 and c['cout'] in (64, 96, 128, 192) and
             c['hs'] % ts(c) == 0 and c['ws'] % ts(c) == 0 and c['w_h2_ptr'] and c['out_ptr']]
    has = lambda pred: any(pred(c) for c in alone)
    plain = lambda c: (c['up'], c['pool'], c['zins'], c['stride']) == (1, 1, 1, 1)
    assert has(lambda c: c['up'] == 2 and c['dact_z_ptr']) and has(lambda c: c['up'] == 2 and c['act_in'] == 1)
    assert has(lambda c: c['pool'] == 2 and c['res_ptr']) and has(lambda c: c['pool'] == 2 and c['bias_ptr']) and has(lambda c: c['pool'] == 2 and c['ln_ptr'])
    for mode in ('zins', 'stride'):
        assert has(lambda c: c[mode] == 2 and c['dact_z_ptr']) and has(lambda c: c[mode] == 2 and c['ln_ptr']) and has(lambda c: c[mode] == 2 and c['act_in'] == 1)
    assert has(lambda c: plain(c) and c['mod_ptr'] and not c['ln_ptr']) and has(lambda c: plain(c) and c['ln_ptr'] and c['act_in'] == 1)
    assert has(lambda c: plain(c) and c['act_in'] == 2 and not c['ln_ptr'])
    assert has(lambda c: plain(c) and c['dact_z_ptr'] and c['act_d'] == 2 and not c['res_ptr'])
    assert has(lambda c: plain(c) and c['dact_z_ptr'] and c['act_d'] == 1 and c['res_ptr'])


def test_null_descriptor_is_unsupported(emu, kernel):
    pick_fn, _, _, _, cases, nout = kernel
    null = [c for c in cases if c['extra'] is None and all(c['switches'])]
    assert null and all(c['rc'] == -2 for c in null)                     # (SDA_E_UNSUPPORTED: what both launch paths returned)
    out = (ctypes.c_int * nout)()
    assert getattr(emu, pick_fn)(None, *null[0]['switches'], 256, out) == -2
