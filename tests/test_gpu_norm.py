"""GPU: every LayerNorm kernel of csrc/norm.hip at its tails, in the call forms the engine uses, against float64.

The cases are tests/norm_cases.py's (tests/test_norm_cases_host.py proves that they reach every instantiation with a partial last
workgroup, dead lanes in the last wavefront and, on the quad kernels, two images inside one wavefront).  Every operand is a view 64
floats into a NaN-filled buffer with 64 floats behind it; afterwards the bands of every written buffer are still NaN and the view
holds none.  The tolerance of a case is tests/norm_ref.py's: 4 x the error of the plain sequential fp32 evaluation on that case's own
inputs, at least 2 fp32 ulps of the tensor's scale.

Measured on an MI355X (88 cases + the refusals: 89 tests, 10.2 s for the file; the slowest case 0.6 s, float64 reference included).
Largest error per family, the sequential fp32 yardstick on the same case, and the largest error / yardstick ratio of any case of the
family (the bound is 4; errors are relative to max |mean|, elementwise relative for rstd, relative to max |gx|):

    entry  family            quantity  largest error  yardstick there  worst ratio
    stats  wave              mean      1.3e-07        5.1e-07          1.00
    stats  wave              rstd      2.8e-05        2.8e-05          1.00      (c = 2, unbiased: one pixel with a tiny variance)
    stats  quad              mean      1.9e-07        5.2e-07          0.36
    stats  quad              rstd      7.2e-06        7.2e-06          1.00      (1000 + randn: the fp32 rounding of x + mod, in both)
    stats  quad, 4 waves     mean      2.1e-07        9.9e-07          0.27
    stats  quad, 4 waves     rstd      2.8e-06        2.7e-06          1.03
    stats  register          mean      6.9e-07        6.9e-07          1.00
    stats  register          rstd      4.7e-06        4.7e-06          1.00
    stats  thread per pixel  mean      1.3e-06        1.3e-06          1.00
    stats  thread per pixel  rstd      7.8e-06        7.8e-06          1.00
    bwd    wave              gx        3.3e-05        3.3e-05          1.02      (c = 2, as above: rstd up to 316 multiplies the roundings)
    bwd    quad              gx        2.7e-06        2.7e-06          1.09
    bwd    split             gx        2.0e-06        2.0e-06          1.14
    bwd    thread per pixel  gx        9.3e-06        9.3e-06          1.00

No case needs more than 1.14 x the yardstick: no kernel is less accurate than the plain sequential loop, the tree-summed means are 3 - 5
times closer to float64.  Local mutations of csrc/norm.hip tried against this file (the three older LN tests of test_gpu_ops.py pass
under each): the modulation row of a wavefront's first image for the whole wavefront -> 18 cases fail (every quad case with a
per-image row); `/ c` for `/ (c - 1)` in ln_bwd_split_kernel<8, 48, 1> -> its unbiased case fails; E[v^2] - m^2 in
ln_stats_quad_kernel<8, 12> -> its 1000 + randn case fails (each statistics kernel has one).  Dropping `&& live` from the quad store
guard changes no output and no test can see it: a dead lane is clamped to quad 0, loads quad 0's operands, and would store quad 0's own
values over themselves (it only runs at all under sda_ln_bwd_amax) -- the guard saves stores, it does not protect memory.
"""
import pytest
import torch

from tests import norm_cases as C
from tests import norm_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-5
BAND = 64
BADARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


class Banded:
    """A device view `BAND + off` floats into a NaN-filled buffer, `BAND` floats (at least) behind it."""

    def __init__(self, dev, shape, off=0, src=None):
        numel = 1
        for s in shape:
            numel *= s
        self.buf = torch.full((numel + 2 * BAND + 4,), float('nan'), device=dev)
        self.lo, self.hi = BAND + off, BAND + off + numel
        self.view = self.buf[self.lo:self.hi].view(shape)
        assert self.buf.data_ptr() % 16 == 0 and (self.view.data_ptr() % 16 == 0) == (off % 4 == 0)
        if src is not None:
            self.view.copy_(src)

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.isnan(self.buf[:self.lo]).all() and torch.isnan(self.buf[self.hi:]).all(), f'{what}: written outside its view'
        assert not torch.isnan(self.view).any(), f'{what}: NaN (or nothing) inside its view'
        return self.view.cpu()


def _inputs(case, seed):
    """CPU operands of a case: x, the flat modulation row as the kernel's pointer sees it, res, gh."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w, pool = case['n'], case['c'], case['h'], case['w'], case['pool']
    x = torch.randn(n, c, h, w, generator=g)
    x = x + 1000 if case['cond'] == 'offset' else x * 3 + 1
    rows = {'none': 0, 'image': n, 'column': n, 'shared': 1}[case['mod']]
    mod = torch.randn(rows * (R.mod_sn(case['mod'], c) or c), generator=g) if rows else None
    res = torch.randn(n, c, h, w, generator=g) if case['res'] else None
    gh = torch.randn(n, c, h * pool[0], w * pool[1], generator=g) if case['entry'] == 'bwd' else None
    return x, mod, res, gh


def _mod_dev(dev, case, mod):
    """The modulation on the device in the case's form; a 'column' view starts COLUMN_START floats in (4-byte aligned only)."""
    if mod is None:
        return None
    off = R.COLUMN_START if case['mod'] == 'column' else 0
    return Banded(dev, (mod.numel(),), off, mod).view


def _report(case, what, err, yard):
    print(f"NORMERR {C.family(C.case_route(case))} {case['entry']} {what} {C.case_id(case)} err={err:.3e} yardstick={yard:.3e} "
          f"ratio={err / max(yard, R.ULP32 / 2):.2f}")


CASE_IDS = [C.case_id(c) for c in C.CASES]
STATS = [i for i, c in enumerate(C.CASES) if c['entry'] == 'stats']
BWD = [i for i, c in enumerate(C.CASES) if c['entry'] == 'bwd']


@pytest.mark.parametrize('idx', STATS, ids=[CASE_IDS[i] for i in STATS])
def test_ln_stats_case(dev, idx):
    from sda_amd import ops
    case = C.CASES[idx]
    n, c, h, w = case['n'], case['c'], case['h'], case['w']
    x, mod, _, _ = _inputs(case, 1000 + idx)
    sn = R.mod_sn(case['mod'], c)
    xb = Banded(dev, x.shape, 1 if case['misaligned'] == 'x' else 0, x)
    md = _mod_dev(dev, case, mod)

    def run(xv, m, m_sn):
        mean = Banded(dev, (n * h * w,), 1 if case['misaligned'] == 'mean' else 0)
        rstd = Banded(dev, (n * h * w,))
        ops.ln_stats(xv, m, m_sn, EPS, case['unbiased'], mean.view, rstd.view)
        return mean, rstd, mean.check('mean'), rstd.check('rstd')

    mean_b, rstd_b, mean, rstd = run(xb.view, md, sn)
    assert torch.equal(xb.check('x'), x)
    mean64, rstd64 = R.stats64(x, mod, case['mod'], EPS, case['unbiased'])
    mean32, rstd32 = R.stats32_seq(x, mod, case['mod'], EPS, case['unbiased'])
    em, ym = R.scale_err(mean, mean64), R.scale_err(mean32, mean64)
    er, yr = R.rel_err(rstd, rstd64), R.rel_err(rstd32, rstd64)
    _report(case, 'mean', em, ym)
    _report(case, 'rstd', er, yr)
    assert em <= R.bound(ym), f'mean: {em:.3e} against a sequential fp32 error of {ym:.3e}'
    assert er <= R.bound(yr), f'rstd: {er:.3e} against a sequential fp32 error of {yr:.3e}'

    if mod is not None:
        # every kernel forms x + mod in fp32 first and the build does not contract: the same call on the materialised sum is bit-identical
        xm = x + R.mod_rows(mod, case['mod'], n, c)[:, :, None, None]
        assert xm.dtype == torch.float32
        xmb = Banded(dev, x.shape, 1 if case['misaligned'] == 'x' else 0, xm)
        _, _, mean_m, rstd_m = run(xmb.view, None, 0)
        assert torch.equal(mean_m, mean) and torch.equal(rstd_m, rstd), 'modulation indexing: differs from the materialised x + mod'

    if case['apply']:
        # one kernel, elementwise: (x + mod - mean) * rstd on the device statistics, bit for bit what fp32 gives on the host
        y = Banded(dev, x.shape)
        ops.ln_apply(xb.view, md, sn, mean_b.view, rstd_b.view, y.view)
        u = x if mod is None else x + R.mod_rows(mod, case['mod'], n, c)[:, :, None, None]
        want = (u - mean.view(n, 1, h, w)) * rstd.view(n, 1, h, w)
        assert torch.equal(y.check('y'), want)
        mean_b.check('mean after apply'), rstd_b.check('rstd after apply')


@pytest.mark.parametrize('idx', BWD, ids=[CASE_IDS[i] for i in BWD])
def test_ln_bwd_case(dev, idx):
    from sda_amd import ops
    case = C.CASES[idx]
    n, c, h, w, pool = case['n'], case['c'], case['h'], case['w'], case['pool']
    x, mod, res, gh = _inputs(case, 1000 + idx)
    sn = R.mod_sn(case['mod'], c)
    # the float64 statistics, rounded to fp32: the backward kernels are judged on their own
    mean, rstd = (t.float() for t in R.stats64(x, mod, case['mod'], EPS, case['unbiased']))
    xb = Banded(dev, x.shape, 1 if case['misaligned'] == 'x' else 0, x)
    mb = Banded(dev, mean.shape, 1 if case['misaligned'] == 'mean' else 0, mean)
    rb, gb = Banded(dev, rstd.shape, 0, rstd), Banded(dev, gh.shape, 0, gh)
    resb = Banded(dev, x.shape, 0, res) if res is not None else None
    md = _mod_dev(dev, case, mod)

    def run(amax=None):
        gx = Banded(dev, x.shape, 1 if case['misaligned'] == 'gx' else 0)
        ops.ln_bwd(gb.view, xb.view, h, w, md, sn, mb.view, rb.view, case['unbiased'], pool, None if resb is None else resb.view, gx.view,
                   out_amax=amax)
        return gx.check('gx')

    gx = run()
    for b, t, name in ((xb, x, 'x'), (mb, mean, 'mean'), (rb, rstd, 'rstd'), (gb, gh, 'gh')):
        assert torch.equal(b.check(name), t)
    gx64 = R.bwd64(gh, x, mod, mean, rstd, case['unbiased'], pool, res, case['mod'])
    gx32 = R.bwd32_seq(gh, x, mod, mean, rstd, case['unbiased'], pool, res, case['mod'])
    e, y = R.scale_err(gx, gx64), R.scale_err(gx32, gx64)
    _report(case, 'gx', e, y)
    assert e <= R.bound(y), f'gx: {e:.3e} against a sequential fp32 error of {y:.3e}'

    if case['amax']:
        # sda_ln_bwd_amax: the same gx, and max |gx| exactly -- over a stale larger value, with dead lanes in the wavefront maximum
        am = Banded(dev, (4,), 0, torch.full((4,), 1e30))
        gx2 = run(am.view)
        got = am.check('amax')
        assert torch.equal(gx2, gx)
        assert float(got[0]) == float(gx.abs().max()) and (got[1:] == 1e30).all()


def test_ln_refusals(dev):
    lib = __import__('sda_amd._lib', fromlist=['load']).load()
    n, c, h, w = 2, 4, 1, 8
    x = torch.randn(n, c, h, w, device=dev)
    mean, rstd = torch.full((n * h * w,), float('nan'), device=dev), torch.full((n * h * w,), float('nan'), device=dev)
    gx = torch.full_like(x, float('nan'))
    p = lambda t: t.data_ptr()
    one = torch.randn(n, 1, h, w, device=dev)
    assert lib.sda_ln_stats(p(one), n, 1, h * w, None, 0, EPS, 1, p(mean), p(rstd), None) == UNSUPPORTED     # unbiased variance of one channel
    assert lib.sda_ln_stats(p(one), n, 1, h * w, None, 0, EPS, 0, p(mean), p(rstd), None) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(mean).any()
    gh = torch.randn(n, c, 2 * h, w, device=dev)
    assert lib.sda_ln_bwd(p(gh), p(x), n, c, h, w, None, 0, p(mean), p(rstd), 1, 2, 1, None, p(gx), None) == UNSUPPORTED   # pool (2, 1)
    assert lib.sda_ln_bwd_amax(p(x), p(x), n, c, h, w, None, 0, p(mean), p(rstd), 1, 1, 1, None, p(gx), None, None) == BADARG
    torch.cuda.synchronize()
    assert torch.isnan(gx).all()                                                 # (a refused call launches nothing that writes gx)
