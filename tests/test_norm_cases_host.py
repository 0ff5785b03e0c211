"""CPU: the case table of tests/test_gpu_norm.py against csrc/norm.hip.

tests/norm_cases.py restates the dispatch of sda_ln_stats / ln_bwd_launch; here every restated constant and table row is read back
from the source text, the set of instantiations route() can name is compared with the kernel names in the built object, every
instantiation must be reached by a case of each required call form, every case on a quad / register / split kernel must leave a
partial last workgroup and every quad case an image boundary inside a wavefront.  The float64 reference (tests/norm_ref.py) is
checked against torch.var_mean and float64 autograd."""
import os
import re
import sys

import pytest
import torch

from tests import norm_cases as C
from tests import norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'sda_amd', 'csrc', 'norm.hip')


@pytest.fixture(scope='module')
def text():
    with open(SRC) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------ constants

@pytest.mark.parametrize('name', ['LN_THREADS', 'LN_SMALL_PIXELS', 'LN_BWD_SMALL_PIXELS', 'LN_QUAD_CMIN', 'LN_QUAD_CMAX', 'LN_REG_C'])
def test_constants_equal_the_source(text, name):
    found = re.findall(rf'^#define {name} (\d+)\s*(?://.*)?$', text, re.M)
    assert len(found) == 1, (name, found)
    assert int(found[0]) == getattr(C, name)


def test_layout_table_equals_the_source(text):
    body = re.search(r'\} LN_QUAD\[\] = \{(.*?)\n\};', text, re.S).group(1)
    rows = re.findall(r'^\s*\{(\d+), ln_stats_quad_launch<([\d, ]+)>, ln_bwd_quad_launch<([\d, ]+)>, ln_bwd_quad_launch<([\d, ]+)>\},', body, re.M)
    assert len(rows) == len([l for l in body.split('\n') if l.strip().startswith('{')])          # (no row in another spelling)
    ints = lambda s: tuple(int(v) for v in s.split(','))
    got = []
    for cmax, st, bw, up in rows:
        st, bw, up = ints(st), ints(bw), ints(up)
        assert len(st) in (2, 3) and len(bw) == 2 and len(up) == 3 and up[2] == 2
        got.append((int(cmax), st + (1,) * (3 - len(st)), bw + (1,), up))                        # (the templates' defaults: NW = 1, POOL = 1)
    assert got == C.LN_QUAD
    assert [r[0] for r in got] == sorted(r[0] for r in got) and got[-1][0] == C.LN_QUAD_CMAX


def test_split_and_register_picks_equal_the_source(text):
    body = re.search(r'static void ln_bwd_split_pick\(const ln_bwd_args& a\) \{(.*?)\n\}', text, re.S).group(1)
    picks = re.findall(r'(?:if \(a\.c <= (\d+)\)|else) ln_bwd_split_launch<(\d+), (\d+), POOL>\(a\);', body)
    assert [(int(b) if b else None, (int(s), int(k))) for b, s, k in picks] == C.LN_SPLIT
    assert len(picks) == body.count('ln_bwd_split_launch<')
    assert 'else if (c > LN_REG_C / 2 && c <= 4 * LN_REG_C && blocks * 4 <= 0x7fffffffLL) {' in text
    reg = re.findall(r'(?:if \(c <= (?:(\d+) \* )?LN_REG_C\)|else) ln_stats_reg_launch<(\d+)>\(a\);', text)
    assert [int(s) for _, s in reg] == list(C.LN_REG_SPLITS) and [b for b, _ in reg] == ['', '2', '']
    # the conditions around the table, as route() states them
    for line in ('if (npix < LN_SMALL_PIXELS) {',
                 'if (quad_on && hw % 4 == 0 && c > LN_QUAD_CMIN && c <= LN_QUAD_CMAX && ln_aligned16(x, mean, rstd)) ln_quad_pick(c).stats(a);',
                 'const bool small = npix < LN_BWD_SMALL_PIXELS;',
                 'const bool wide = shape != 12 && c > LN_QUAD_CMIN && c <= LN_QUAD_CMAX;',
                 'if (!small && wide && quad_on && (shape == 11 ? (h * w) % 4 == 0 : w % 4 == 0) && ln_aligned16(gh, x, gx, mean, rstd, res)) {',
                 '} else if (!small && wide && blocks * 8 <= 0x7fffffffLL) {'):
        assert line in text, line


# ------------------------------------------------------------------------------------------------------------ kernel names

def _object_kernels():
    """(function, template integers) of every ln_* kernel in the built object -- names only."""
    from sda_amd import build as sbuild
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_guard as G
    sbuild.build()
    out = set()
    for name in G.kernel_metadata(os.path.join(sbuild.LIBDIR, 'norm.o')):
        m = re.match(r'_Z\d+(ln_[a-z_]+_kernel)(?:I((?:Li\d+E)+)E)?v?P', name)
        assert m, name
        out.add((m.group(1), tuple(int(v) for v in re.findall(r'Li(\d+)E', m.group(2) or ''))))
    return out


def test_routable_set_is_the_objects_kernel_set():
    want = {C.kernel_name(r) for r in C.routable()}
    assert len(want) == len(C.routable())
    assert _object_kernels() == want


# ------------------------------------------------------------------------------------------------------------ coverage

def _is(case, form):
    return all(case[k] == v for k, v in form.items() if not (case['entry'] == 'stats' and k == 'res'))


def test_every_instantiation_has_both_required_forms():
    routes = [r for r in C.routable() if r not in (('apply',), ('amax_zero',))]
    assert len(routes) == 32
    for r in sorted(routes):
        mine = [c for c in C.CASES if C.case_route(c) == r]
        for form in (C.FORM_A, C.FORM_B):
            want = {k: form[k] for k in ('mod', 'res', 'unbiased')}
            assert any(_is(c, want) for c in mine), (r, want)
        if r[0].startswith('stats'):
            # "two-pass, no E[x^2] - m^2 cancellation" is a claim about each statistics kernel: each one sees 1000 + randn
            assert any(c['cond'] == 'offset' for c in mine), r
        if r[0] in ('stats_quad', 'bwd_quad', 'stats_reg', 'bwd_split'):
            # the row's widest width and a ragged one inside it
            widest = max(c for c in range(1, C.LN_QUAD_CMAX + 1)
                         if C.route(mine[0]['entry'], 3, c, 1, 5468 if 'quad' in r[0] else 5469, mine[0]['pool']) == r)
            assert any(c['c'] == widest for c in mine) and any(c['c'] < widest for c in mine), (r, widest)


def test_every_family_has_shared_image_and_offset():
    for entry, fams in (('stats', ('wave', 'quad', 'quad_nw4', 'split', 'plain')), ('bwd', ('wave', 'quad', 'split', 'plain'))):
        for fam in fams:
            mine = [c for c in C.CASES if c['entry'] == entry and C.family(C.case_route(c)) == fam]
            assert {'shared', 'image', 'column', 'none'} <= {c['mod'] for c in mine}, (entry, fam)
            assert any(c['cond'] == 'offset' for c in mine) and any(c['cond'] == 'plain' for c in mine), (entry, fam)
            assert {True, False} == {c['unbiased'] for c in mine}, (entry, fam)


def test_apply_amax_and_misaligned_cases():
    assert sorted(c['mod'] for c in C.CASES if c['apply']) == sorted(C.MOD_FORMS)
    amax = {c['amax']: C.case_route(c) for c in C.CASES if c['amax']}
    assert set(amax) == {'lanes8', 'lanes16', 'pooled', 'fallback'}
    assert amax['lanes8'][:2] == ('bwd_quad', 8) and amax['lanes8'][3] == 1
    assert amax['lanes16'][:2] == ('bwd_quad', 16) and amax['lanes16'][3] == 1
    assert amax['pooled'][0] == 'bwd_quad' and amax['pooled'][3] == 2
    assert amax['fallback'][0] == 'bwd_split'
    assert all(C.tail(c) for c in C.CASES if c['amax'])                      # (dead lanes take part in the wavefront maximum)
    mis = [c for c in C.CASES if c['misaligned']]
    assert {(c['entry'], c['misaligned']) for c in mis} == {('stats', 'x'), ('stats', 'mean'), ('bwd', 'x'), ('bwd', 'gx'), ('bwd', 'mean')}
    for c in mis:
        # eligible for the quad path but for the pointer, and sent to the register / split kernels
        assert C.route(c['entry'], c['n'], c['c'], c['h'], c['w'], c['pool'], True)[0] in ('stats_quad', 'bwd_quad')
        assert C.case_route(c)[0] in ('stats_reg', 'bwd_split')
    one_by_two = [c for c in C.CASES if c['pool'] == (1, 2)]
    assert any(C.case_route(c) == ('bwd_plain', 1, 2) and c['c'] == 96 for c in one_by_two)
    assert any(C.case_route(c) == ('bwd_wave', 1, 2) for c in one_by_two)


def test_case_ids_are_unique_and_the_table_stays_small():
    ids = [C.case_id(c) for c in C.CASES]
    assert len(set(ids)) == len(ids)
    assert 60 <= len(ids) <= 90
    for c in C.CASES:
        assert not (c['unbiased'] and c['c'] < 2)


# ------------------------------------------------------------------------------------------------------------ tails

def test_every_grouped_case_has_a_tail_and_every_quad_case_a_straddling_wavefront():
    seen = 0
    for c in C.CASES:
        r = C.case_route(c)
        if C.units_per_workgroup(r)[0] is None:
            continue
        seen += 1
        assert C.tail(c) != 0, C.case_id(c)
        if r[0] in ('stats_quad', 'bwd_quad'):
            assert (c['h'] * c['w']) % 4 == 0 and C.straddles(c), C.case_id(c)
            qw = 64 // r[1]
            assert (c['n'] * c['h'] * c['w'] // 4) % qw != 0, C.case_id(c)      # (dead lanes inside the last live wavefront too)
    assert seen >= 40
    # the tail arithmetic itself, on shapes whose answer is known
    full = dict(entry='stats', n=4, c=96, h=64, w=64, pool=(1, 1), misaligned=None)
    assert C.tail(full) == 0 and not C.straddles(full)
    assert C.tail(dict(full, n=3, h=1, w=5468)) == 4101 % 32 == 5 and C.straddles(dict(full, n=3, h=1, w=5468))
    assert C.tail(dict(full, n=3, h=1, w=5468, c=384)) == 4101 % 8 == 5
    assert C.tail(dict(full, n=3, h=1, w=5469)) == 16407 % 256
    for c in C.CASES:                                                            # the other kernels: a partial last workgroup as well
        r = C.case_route(c)
        npix = c['n'] * c['h'] * c['w']
        if r[0] in ('stats_plain', 'bwd_plain'):
            assert npix % C.LN_THREADS != 0
        if r[0] in ('stats_wave', 'bwd_wave'):
            assert npix % (C.LN_THREADS // 64) != 0


# ------------------------------------------------------------------------------------------------------------ reference

@pytest.mark.parametrize('unbiased', [True, False])
@pytest.mark.parametrize('kind', C.MOD_FORMS)
def test_stats64_is_var_mean(kind, unbiased):
    torch.manual_seed(1)
    n, c, h, w = 2, 5, 3, 4
    x = torch.randn(n, c, h, w) * 3 + 1
    mod = torch.randn(n * (c + R.COLUMN_PAD))
    mean, rstd = R.stats64(x, mod, kind, 1e-5, unbiased)
    rows = R.mod_rows(mod, kind, n, c)
    u = x.double() if rows is None else x.double() + rows.double()[:, :, None, None]
    if kind == 'shared':
        assert torch.equal(rows[0], rows[1])
    if kind == 'column':
        assert torch.equal(rows[1], mod[c + R.COLUMN_PAD:2 * c + R.COLUMN_PAD])
    var, m = torch.var_mean(u, dim=1, unbiased=unbiased)
    assert (mean - m.reshape(-1)).abs().max() <= 1e-12
    assert (rstd - (var + 1e-5).rsqrt().reshape(-1)).abs().max() <= 1e-12
    m32, r32 = R.stats32_seq(x, mod, kind, 1e-5, unbiased)
    assert m32.dtype == torch.float32 and R.scale_err(m32, mean) < 1e-6 and R.rel_err(r32, rstd) < 1e-6


@pytest.mark.parametrize('unbiased', [True, False])
@pytest.mark.parametrize('pool', [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize('with_res', [True, False])
def test_bwd64_is_float64_autograd(pool, unbiased, with_res):
    torch.manual_seed(2)
    n, c, h, w = 2, 5, 3, 4
    x = torch.randn(n, c, h, w) * 3 + 1
    mod = torch.randn(n * c)
    res = torch.randn(n, c, h, w) if with_res else None
    gh = torch.randn(n, c, h * pool[0], w * pool[1])
    mean, rstd = R.stats64(x, mod, 'image', 1e-5, unbiased)
    xd = x.double().requires_grad_(True)
    u = xd + mod.double().reshape(n, c, 1, 1)
    var, m = torch.var_mean(u, dim=1, unbiased=unbiased, keepdim=True)
    hup = ((u - m) / torch.sqrt(var + 1e-5)).repeat_interleave(pool[1], -1).repeat_interleave(pool[0], -2)
    want, = torch.autograd.grad(hup, xd, gh.double())
    if with_res:
        want = want + res.double()
    got = R.bwd64(gh, x, mod, mean, rstd, unbiased, pool, res)
    assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-12
    # it takes the statistics it is given
    other = R.bwd64(gh, x, mod, mean + 0.5, rstd, unbiased, pool, res)
    assert (other - want).abs().max() > 1e-3
    g32 = R.bwd32_seq(gh, x, mod, mean.float(), rstd.float(), unbiased, pool, res)
    assert g32.dtype == torch.float32 and R.scale_err(g32, R.bwd64(gh, x, mod, mean.float(), rstd.float(), unbiased, pool, res)) < 1e-6


def test_bound_and_error_measures():
    assert R.bound(0.0) == 2 * 2.0 ** -23 and R.bound(1e-6) == 4e-6
    ref = torch.tensor([1000.0, 1.0])
    assert R.scale_err(ref + torch.tensor([0.0, 1e-3]), ref) == pytest.approx(1e-6, rel=1e-3)
    assert R.rel_err(ref + torch.tensor([0.0, 1e-3]), ref) == pytest.approx(1e-3, rel=1e-3)
    assert R.scale_err(torch.zeros(3), torch.zeros(3)) == 0.0


# ------------------------------------------------------------------------------------------------------------ the host shim

def test_cpu_shim_ln_bwd_writes_amax(monkeypatch):
    """tests/cpu_shim.py stands in for ops.ln_bwd on the host: with out_amax it reports max |gx|, as sda_ln_bwd_amax does."""
    from sda_amd import ops
    from tests import cpu_shim
    cpu_shim.install(monkeypatch)
    torch.manual_seed(3)
    n, c, h, w = 2, 6, 2, 4
    x, gh, res = torch.randn(n, c, h, w), torch.randn(n, c, 2 * h, 2 * w), torch.randn(n, c, h, w)
    mod = torch.randn(n, c)
    mean, rstd = (t.float() for t in R.stats64(x, mod.reshape(-1), 'image', 1e-5, True))
    gx, amax = torch.empty_like(x), torch.full((1,), 1e30)
    ops.ln_bwd(gh, x, h, w, mod, c, mean, rstd, True, (2, 2), res, gx, out_amax=amax)
    assert float(amax[0]) == float(gx.abs().max())
    assert R.scale_err(gx, R.bwd64(gh, x, mod.reshape(-1), mean, rstd, True, (2, 2), res)) < 1e-5
