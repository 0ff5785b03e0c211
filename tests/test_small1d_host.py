"""CPU: the planner of csrc/conv_small1d.hip through sda_small1d_tile (host only, nothing is launched), the case table of
tests/small1d_cases.py against it -- so every case of tests/test_gpu_small1d.py provably reaches the kernel instance it names -- and
the float64 reference of tests/small1d_ref.py against torch."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import small1d_cases as K
from tests import small1d_ref as R
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG = -1


def desc(n=4, length=100, cx=40, cin_pad=40, cout=40, cout_pad=64, **over):
    """An eligible descriptor with made-up, never followed addresses; `over`: raw field values set last."""
    from sda_amd.ops import make_conv_desc
    d = make_conv_desc(x_ptr=0x10000, n=n, cx=cx, hs=1, ws=length, x_sc=length, x_sy=length, x_sx=1, x_sn_outer=cx * length, w_ptr=0x20000,
                       cin_pad=cin_pad, cout_pad=cout_pad, cout=cout, kh=1, kw=3, out_ptr=0x30000, ho=1, wo=length, mt=cout_pad // 32 or 1)
    for f, v in over.items():
        setattr(d, f, v)
    return d


def tile_of(d):
    from sda_amd import _lib, ops
    raw = _lib.load().sda_small1d_tile(ctypes.byref(d))
    if raw >= 0:
        assert ops.small1d_tile(d) == raw
    return raw


@pytest.fixture(autouse=True)
def _plain_environment():
    """The planner reads its two switches once per process: this module's expectations hold without them."""
    assert os.environ.get('SDA_SMALL1D_TP') is None and os.environ.get('SDA_CONV_SMALL1D') is None


@pytest.mark.parametrize('n,wo,tile', [(512, 32, 16), (513, 32, 32), (1024, 32, 32), (1025, 32, 64), (1025, 1, 64), (4096, 64, 64),
                                       (4097, 64, 0)])
def test_planner_boundaries(n, wo, tile):
    """16 while n * ceil(wo / 16) <= 1024, else 32 while n * ceil(wo / 32) <= 1024, else 64; 0 once n * ceil(wo / tile) > 4096."""
    want = 16 if n * -(-wo // 16) <= 1024 else 32 if n * -(-wo // 32) <= 1024 else 64
    if n * -(-wo // want) > 4096:
        want = 0
    assert want == tile == K.plan(n, wo)
    d = desc(n=n, length=wo)
    assert tile_of(d) == tile
    from sda_amd import ops
    assert ops.conv_path(d) == (3 if tile else 0)


def test_planner_formula_on_a_sweep():
    """small1d_cases.plan against the library over both thresholds and the cap, long single sequences included."""
    for n, wo in [(n, wo) for n in (1, 2, 63, 64, 65, 256, 341, 342, 511, 512, 513, 1024, 1025, 2048, 4096, 4097, 70000)
                  for wo in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 128, 129)] + [(1, 16384), (1, 16385), (1, 32768), (1, 32769),
                                                                                      (1, 262144), (1, 262145)]:
        assert tile_of(desc(n=n, length=wo)) == K.plan(n, wo), (n, wo)


DECLINED = [dict(kh=3), dict(kw=1), dict(kw=5), dict(stride_h=2), dict(stride_w=2), dict(hs=2), dict(ho=2), dict(up_h=2), dict(up_w=2),
            dict(zins_h=2), dict(zins_w=2), dict(cctx=1), dict(explicit_pad=1), dict(out_sn=4000), dict(out_sc=100), dict(out_sy=100),
            dict(out_sx=1), dict(cin_pad=68, cx=68), dict(cin_pad=68), dict(cin_pad=6, cx=6), dict(cout_pad=80, cout=80), dict(cout_pad=80),
            dict(cout_pad=24, cout=24), dict(cx=41), dict(cout=65), dict(wo=99), dict(ws=99), dict(wo=0, ws=0), dict(n=0), dict(n_inner=0),
            dict(x=None), dict(w=None), dict(out=None)]


@pytest.mark.parametrize('bad', DECLINED, ids=lambda b: '-'.join(f'{k}{v}' for k, v in b.items()))
def test_declined_descriptors(bad):
    """Every field the plan declines on, one at a time: 0, the launch goes to the general kernels (and is not reported as path 3)."""
    from sda_amd import ops
    assert tile_of(desc()) == 16
    d = desc(**bad)
    assert tile_of(d) == 0
    assert ops.conv_path(d) != 3


@pytest.mark.parametrize('good', [dict(cin_pad=64, cx=64), dict(cin_pad=4, cx=3), dict(cout_pad=16, cout=1), dict(cout_pad=48, cout=33),
                                  dict(cout_pad=64, cout=64), dict(x_sx=40, x_sc=1), dict(n_inner=5, x_sn_inner=7), dict(x_n_off=3),
                                  dict(circular=1), dict(act_in=3, act_d=3), dict(mod=0x40000, mod_sn=40), dict(bias=0x40000),
                                  dict(dact_z=0x40000), dict(res=0x40000), dict(ln_mean=0x40000, ln_rstd=0x50000)],
                         ids=lambda b: '-'.join(f'{k}{v}' for k, v in b.items()))
def test_served_descriptors(good):
    """The other side of every refusal: the widest and narrowest paddings, every source view and every fusion are served."""
    assert tile_of(desc(**good)) == 16


def test_bad_descriptors():
    from sda_amd import _lib, ops
    assert _lib.load().sda_small1d_tile(None) == 0
    for half in (dict(ln_mean=0x40000), dict(ln_rstd=0x40000)):
        d = desc(**half)
        assert tile_of(d) == E_BADARG
        with pytest.raises(_lib.SdaHipError):
            ops.small1d_tile(d)
    # (a refusal comes first: what the kernel does not take is the general kernels' to judge)
    assert tile_of(desc(ln_mean=0x40000, kw=5)) == 0


_PROBE = ('import ctypes, sys; sys.path.insert(0, {root!r}); from tests.test_small1d_host import desc; from sda_amd import _lib, ops; '
          'print([(_lib.load().sda_small1d_tile(ctypes.byref(desc(n=n, length=wo))), ops.conv_path(desc(n=n, length=wo))) for n, wo in {shapes!r}])')


def _probe(shapes, **env):
    out = subprocess.run([sys.executable, '-c', _PROBE.format(root=ROOT, shapes=shapes)], cwd=ROOT, env=dict(os.environ, **env),
                         stdout=subprocess.PIPE, timeout=120, check=True).stdout.decode()
    return eval(out.strip().splitlines()[-1])


SHAPES = [(4, 100), (600, 20), (1025, 5), (257, 16), (4096, 16), (4097, 16), (4096, 64), (4096, 65), (2048, 128), (2049, 128)]


@pytest.mark.parametrize('env,want', [
    (dict(SDA_CONV_SMALL1D='0'), [(0, 0)] * len(SHAPES)),
    # the forced tile serves what the plan accepts, and its own grid is held to the cap: 4096 x 65 and 2049 x 128 are 8192 / 4098 workgroups
    (dict(SDA_SMALL1D_TP='64'), [(64, 3)] * 5 + [(0, 0), (64, 3), (0, 0), (64, 3), (0, 0)]),
    (dict(SDA_SMALL1D_TP='32'), [(32, 3)] * 5 + [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0)]),
    # 4096 x 64, served unforced on 4096 workgroups of 64 positions, would be 16384 workgroups of 16
    (dict(SDA_SMALL1D_TP='16'), [(16, 3)] * 5 + [(0, 0)] * 5),
    # anything but 16 / 32 / 64 forces nothing
    (dict(SDA_SMALL1D_TP='48'), None), (dict(SDA_SMALL1D_TP='0'), None), (dict(), None),
], ids=['small1d_off', 'tp64', 'tp32', 'tp16', 'tp48_ignored', 'tp0_ignored', 'unset'])
def test_environment_switches(env, want):
    """One child process per switch (each is read once): SDA_CONV_SMALL1D=0 declines everything; SDA_SMALL1D_TP forces the tile of
    the launches the plan accepts and still refuses n * ceil(wo / tile) > 4096."""
    if want is None:
        want = [(K.plan(n, wo), 3 if K.plan(n, wo) else 0) for n, wo in SHAPES]
    else:
        forced = int(env.get('SDA_SMALL1D_TP', 0))
        if forced:
            assert [t for t, _ in want] == [K.plan(n, wo, forced) for n, wo in SHAPES]
    assert _probe(SHAPES, **env) == want


def case_desc(case, lo=0, n=None):
    """The descriptor of a case's launch as the GPU test builds it, with made-up addresses."""
    fz = K.FUSIONS[case['fuse']]
    cin_pad, cout_pad = K.pads(case)
    src = K.source_fields(case, lo, n)
    over = dict(x_sn_outer=src['x_sn_outer'], x_sn_inner=src['x_sn_inner'], n_inner=src['n_inner'], x_n_off=src['x_n_off'], x_sc=src['x_sc'],
                x_sy=src['x_sy'], x_sx=src['x_sx'], circular=int(case['circular']))
    if fz['mod'] != 'none':
        over.update(mod=0x40000, mod_sn=case['cin'] if fz['mod'] == 'image' else 0)
    if fz['ln']:
        over.update(ln_mean=0x50000, ln_rstd=0x60000)
    over.update(act_in=R_ACT[fz['act']], act_d=R_ACT[fz['dact']])
    for on, field in ((fz['bias'], 'bias'), (fz['dact'] != 'none', 'dact_z'), (fz['res'], 'res')):
        if on:
            over[field] = 0x70000
    return desc(n=src['n'], length=case['wo'], cx=case['cin'], cin_pad=cin_pad, cout=case['cout'], cout_pad=cout_pad, **over)


R_ACT = {'none': 0, 'SiLU': 1, 'ELU': 3}
ALL_CASES = K.CASES + [K.CROSS]


def test_case_table_is_well_formed():
    ids = [K.case_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    from sda_amd import ops
    for c in ALL_CASES:
        assert 1 <= c['cin'] <= K.MAXC and 1 <= c['cout'] <= K.MAXC
        if c['pack'] == 'own':                               # what PackedConv gives this layer
            assert K.pads(c) == (ops.round_up(c['cin'], ops.CONV_CK), ops.round_up(c['cout'], 32 * ops.pick_mt(c['cout']))), K.case_id(c)
        for lo, n, _ in K.launches(c):
            assert 0 <= lo and lo + n <= c['n']
        if c['view'] == 'split':
            assert sorted((lo, lo + n) for lo, n, _ in c['chunks'])[0][0] == 0 and sum(n for _, n, _ in c['chunks']) == c['n']
            assert all(lo > 0 for lo, _, _ in c['chunks'][1:])
    # what the issue asks of the table: every tile, both paddings per family, each fusion alone and every view on every tile
    for tile in (16, 32, 64):
        mine = [c for c in K.CASES if tile in [t for _, _, t in K.launches(c)]]
        assert {c['fuse'] for c in mine} >= set(K.EACH_FUSION), tile
        assert {c['view'] for c in mine} == set(K.VIEWS), tile
        assert any(c['transpose'] for c in mine), tile
    for family in ('t64_multi', 't64_short', 't32', 't16_edge', 't64_cap'):
        assert {c['circular'] for c in K.CASES if c['family'] == family} == {True, False}, family
    assert {(c['cin'], c['cout']) for c in K.CASES} >= {(64, 64), (17, 33), (3, 64), (64, 1), (40, 16)}
    assert {K.pads(c)[1] for c in K.CASES} == {16, 32, 48, 64}
    assert {c['wo'] for c in K.CASES if c['family'] == 't64_short' and c['view'] == 'planar'} == {1, 2, 3, 5, 16}


@pytest.mark.parametrize('case', ALL_CASES, ids=K.case_id)
def test_every_case_reaches_the_tile_it_names(case):
    from sda_amd import ops
    for lo, n, tile in K.launches(case):
        d = case_desc(case, lo, n)
        assert tile == K.plan(n, case['wo'])
        assert tile_of(d) == tile, (lo, n)
        assert (ops.conv_path(d) == 3) == (tile != 0), (lo, n)


# ------------------------------------------------------------------------------------------ the reference

def _small(case_args, **kw):
    return K._case('t16_edge', 16, *case_args, **kw)


@pytest.mark.parametrize('circular', [False, True])
@pytest.mark.parametrize('shape', [(3, 7, (5, 6)), (2, 1, (3, 4)), (2, 2, (4, 1)), (1, 33, (17, 33))])
def test_reference_equals_conv1d_on_plain_launches(shape, circular):
    n, wo, ch = shape
    case = _small((n, wo, ch, 'circular' if circular else 'zeros'), fuse='bias')
    L = R.make_launch(case)
    x = L['store'].reshape(n, ch[0], wo).double()
    xp = F.pad(x, (1, 1), mode='circular' if circular else 'constant')
    want = F.conv1d(xp, L['w_torch'].double(), L['b'].double())
    got = R.small1d_ref(L)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()


@pytest.mark.parametrize('circular', [False, True])
@pytest.mark.parametrize('shape', [(3, 7, (6, 5)), (2, 1, (4, 3)), (2, 2, (33, 17))])
def test_reference_with_the_transposed_packing_equals_autograd(shape, circular):
    """Backward data: the launch over the cotangent g with the transposed packing is d <conv(x), g> / d x."""
    n, wo, ch = shape                                        # the launch's (cin, cout) = the layer's (cout, cin)
    case = _small((n, wo, ch, 'circular' if circular else 'zeros'), fuse='off', transpose=True)
    L = R.make_launch(case)
    g = L['store'].reshape(n, ch[0], wo).double()
    x = torch.zeros(n, ch[1], wo, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(F.pad(x, (1, 1), mode='circular' if circular else 'constant'), L['w_torch'].double())
    want, = torch.autograd.grad(y, x, g)
    got = R.small1d_ref(L)
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()


def test_reference_fusions_equal_the_composed_torch_ops():
    """Every step on, per-image modulation, written the long way round with torch modules."""
    case = _small((4, 9, (6, 5), 'circular'), fuse='all_image_elu')
    L = R.make_launch(case)
    x = L['store'].reshape(4, 6, 9).double() + L['mod'].double()[:, :, None]
    var, mean = torch.var_mean(x, dim=1, unbiased=True, keepdim=True)
    assert_close(L['ln'][0], mean[:, 0].float(), 2e-6)
    v = F.elu((x - L['ln'][0].double()[:, None]) * L['ln'][1].double()[:, None])
    y = F.conv1d(F.pad(v, (1, 1), mode='circular'), L['w_torch'].double(), L['b'].double())
    z = L['dact_z'].double()
    want = y * torch.where(z > 0, torch.ones_like(z), z.exp()) + L['res'].double()
    got = R.small1d_ref(L)
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()


def test_reference_source_views_and_chunks():
    """Channel-last and window storage give what the materialised tensor gives; a chunk is the slice of the whole launch."""
    cl = _small((4, 9, (6, 5), 'zeros'), fuse='all_image_elu', view='channel_last')
    L = R.make_launch(cl)
    x = L['store'].reshape(4, 9, 6).permute(0, 2, 1)
    assert torch.equal(R.source_view(L['store'], L['src']), x)
    win = _small((27, 9, (10, 5), 'zeros'), fuse='all_image_elu', view='window')
    Lw = R.make_launch(win)
    B, T, C, nw = K.window_geometry(win)
    assert (B, T, C, nw) == (3, 13, 2, 9)
    traj = Lw['store'].reshape(B, T, C, 9)
    want = torch.stack([traj[b, i:i + K.WINDOW].reshape(K.WINDOW * C, 9) for b in range(B) for i in range(nw)])
    assert torch.equal(R.source_view(Lw['store'], Lw['src']), want)
    for launch in (L, Lw):
        whole = R.small1d_ref(launch)
        n = launch['n']
        for lo, cnt in ((0, 1), (1, n - 1), (n // 2, n - n // 2)):
            part = R.small1d_ref(launch, lo=lo, n=cnt)           # (float64 round-off apart: the matrix products batch differently)
            assert part.shape == whole[lo:lo + cnt].shape
            assert (part - whole[lo:lo + cnt]).abs().max().item() <= 1e-13 * whole.abs().max().item()


@pytest.mark.parametrize('case', [c for c in ALL_CASES if c['n'] * c['wo'] * c['cout'] <= 1 << 22], ids=K.case_id)
def test_float32_evaluation_is_well_conditioned(case):
    """The yardstick of the GPU test is usable: the float32 CPU evaluation of every case stays within assert_close's per-element
    criterion at the tolerance derived from its own error (at most 1 element in 1000 outside would be the cap; none is)."""
    L = R.make_launch(case)
    ref64, ref32 = R.small1d_ref(L), R.small1d_ref(L, torch.float32)
    assert ref32.dtype == torch.float32
    yard = R.yardstick(ref64, ref32)
    assert yard < 2.5e-5, f'float32 itself is off by {yard:.2e}: the inputs are ill-conditioned'
    assert_close(ref32, ref64, R.tolerance(yard), what=K.case_id(case))
