"""GPU: the three kernels of csrc/step1d.hip, each alone, through the C ABI.

sda_step1d_prologue   bit for bit against sda_vp_schedule + sda_time_embed + sda_linear_small on the same fp32 inputs, and within
                      tests/step1d_ref.py's bound of float64, at every shape where the kernel takes another path (staged / unstaged, the three
                      projection branches, every load slot, both sides of the LDS bound, the 8-feature floor, tails of sda_dot8 and the
                      split dot product, the maxima, a misaligned weight view), both call forms, the 3 x 3 stock schedules;
sda_pc_correct_keyed  bit for bit against sda_randn_rows + sda_pc_correct at every per_sample % 4, below one quad, on the second
                      grid-stride trip, with row and draw indices on both sides of 2^32; the smallest against float64;
sda_mc_finish         bit for bit against sda_unfold_adjoint + sda_guided_combine (+ sda_pc_predict / sda_sumsq_partial) for a bare network,
                      against float64 for the affine estimator, on both sides of the 16-value row stride switch.
Every output buffer lies between NaN guard bands."""
import math

import numpy as np
import pytest
import torch

from tests import philox_ref, step1d_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
ETA = 1e-3
STOCK_K = (0.0, math.acos(math.sqrt(ETA)), math.log(ETA))          # fused1d.stock_schedule
COS_VP = (1, ETA, STOCK_K[1], 0)
STAGED, UNSTAGED = 1, 0
# rows {t, t - dt, r, c1, sigma(t - dt)} (+ two columns the kernel must step over): t = 1 and t = 0 are among the times
TABLE = [[1.0, 0.8125, 0.97, 0.013, 0.4, 7.0, 8.0], [0.5, 0.37, 0.96, 0.02, 0.3, 7.5, 8.5], [0.013, 0.0, 0.91, 0.05, 0.001, 7.7, 8.7]]
TIMES = [v for row in TABLE for v in row[:2]]

#: worst error / bound seen by the float64 checks of this run, per kernel (printed: CHANGELOG.md quotes them)
RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))
    print(f'step1d {what}: error / bound = {float(ratio):.3f} (worst so far {RATIOS[what]:.3f})')


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from sda_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Guarded:
    """n floats between two NaN guard bands; prefilled with NaN unless `fill` is given."""

    def __init__(self, n, dev, fill=None):
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


# ------------------------------------------------------------------------------------------------------------ prologue
# nf, hidden, e, cp, misaligned wp, expected pick
SHAPES = [
    (16, 256, 32, 192, False, STAGED),          # today's shape: e == 32, the float4 projection branch
    (16, 256, 32, 0, False, STAGED),            # no projection
    (16, 256, 16, 24, False, STAGED),           # e < 32
    (16, 256, 64, 40, False, STAGED),           # a wave per projection output
    (16, 512, 32, 0, False, STAGED),            # all eight load slots of every thread
    (16, 256, 32, 486, False, STAGED),          # the last size within 140 KiB
    (16, 256, 32, 487, False, UNSTAGED),        # ... and the first beyond
    (4, 8, 4, 3, False, STAGED),                # eight input features: the floor
    (2, 8, 4, 3, False, UNSTAGED),
    (13, 100, 24, 7, False, UNSTAGED),          # tails: sda_dot8 at 26 % 8 = 2 and 100 % 8 = 4, the split dot product at 100 % 32 = 4
    (64, 1024, 256, 33, False, UNSTAGED),       # the three maxima; e = 256: four terms per lane
    (16, 256, 32, 192, True, UNSTAGED),         # the staged shape with wp one float into a larger buffer
]
_IDS = ['-'.join(map(str, s[:4])) + ('-misaligned' if s[4] else '') for s in SHAPES]
_cache = {}


def _inputs(dev, nf, hidden, e, cp, misaligned):
    """Seeded fp32 inputs of one shape (torch.nn.Linear's scale, so that pre-activations stay in SiLU's measured range), the unfused
    kernels' results at TIMES and the float64 reference -- computed once per shape and left unchanged."""
    key = (nf, hidden, e, cp)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * nf + hidden + 7 * e + cp)

        def uni(*shape, fan):
            return ((torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan)).to(dev)
        p = dict(freqs=(torch.pi * torch.arange(1, nf + 1)).float().to(dev),
                 w0=uni(hidden, 2 * nf, fan=2 * nf), b0=uni(hidden, fan=2 * nf), w2=uni(e, hidden, fan=hidden), b2=uni(e, fan=hidden),
                 wp=uni(cp, e, fan=e) if cp else None, bp=uni(cp, fan=e) if cp else None)
        if cp:
            big = torch.zeros(cp * e + 8, device=dev)
            big[1:1 + cp * e] = p['wp'].reshape(-1)
            p['wp_off'] = big[1:1 + cp * e].view(cp, e)            # the same values, 4 bytes off a 16-byte boundary
            assert p['wp_off'].data_ptr() % 16 == 4 and p['wp'].data_ptr() % 16 == 0
        p['unfused'] = _unfused(dev, p, TIMES, COS_VP)
        host = {k: v.cpu().numpy() for k, v in p.items() if torch.is_tensor(v) and k != 'wp_off'}
        p['ref'] = R.prologue(np.float32(TIMES), COS_VP, host['freqs'], host['w0'], host['b0'], host['w2'], host['b2'], host.get('wp'),
                              host.get('bp'))
        _cache[key] = p
    p = dict(_cache[key])
    if misaligned:
        p['wp'] = p['wp_off']
    return p


def _unfused(dev, p, times, sched):
    """(coef [nt][2], mod [nt][cp or e]) of the kernels the prologue replaces."""
    from sda_amd import ops
    t = torch.tensor(times, device=dev, dtype=torch.float32)
    ak, eta, k, sk = sched
    coef = torch.stack([ops.vp_schedule(t[i:i + 1], ak, eta, k, sk) for i in range(len(times))])
    mod = ops.time_embed(t, p['freqs'], p['w0'], p['b0'], p['w2'], p['b2'])
    if p['wp'] is not None:
        mod = ops.linear_small(mod, p['wp'].contiguous(), p['bp'])
    return coef, mod


def _width(p):
    return p['wp'].shape[0] if p['wp'] is not None else p['w2'].shape[0]


def _pick(lib, p):
    nf, hidden, e = p['freqs'].numel(), p['w0'].shape[0], p['w2'].shape[0]
    cp = p['wp'].shape[0] if p['wp'] is not None else 0
    return lib.sda_step1d_prologue_path(nf, hidden, e, cp, p['w0'].data_ptr(), p['w2'].data_ptr(), None if cp == 0 else p['wp'].data_ptr())


def _run(lib, dev, p, sched, table=None, istep=None, t=None, nt=2):
    """One launch into NaN-prefilled, guarded buffers -> (coef Guarded [16], mod Guarded [2][width], out_step)."""
    from sda_amd import _lib
    ak, eta, k, sk = sched
    nf, hidden, e = p['freqs'].numel(), p['w0'].shape[0], p['w2'].shape[0]
    cp = p['wp'].shape[0] if p['wp'] is not None else 0
    coef, mod = Guarded(16, dev), Guarded(2 * _width(p), dev)
    out_step = torch.full((1,), -7, device=dev, dtype=torch.int64)
    _lib.check(lib.sda_step1d_prologue(
        None if table is None else table.data_ptr(), 0 if table is None else table.shape[1], None if istep is None else istep.data_ptr(),
        None if t is None else t.data_ptr(), nt, ak, eta, k, sk, p['freqs'].data_ptr(), nf, p['w0'].data_ptr(), p['b0'].data_ptr(), hidden,
        p['w2'].data_ptr(), p['b2'].data_ptr(), e, None if cp == 0 else p['wp'].data_ptr(), None if cp == 0 else p['bp'].data_ptr(), cp,
        coef.ptr(), out_step.data_ptr(), mod.ptr(), _stream()), 'sda_step1d_prologue')
    torch.cuda.synchronize()
    return coef, mod, out_step


def _check_f64(what, got, ref: 'R.V'):
    err = np.abs(got.double().cpu().numpy() - ref.v)
    assert (ref.e > 0).all()
    ratio = (err / ref.e).max()
    _note(what, ratio)
    assert ratio <= 1.0, f'{what}: {ratio:.3f} x the fp32 bound from float64'


@pytest.mark.parametrize('shape', SHAPES, ids=_IDS)
def test_prologue_table_form_is_bit_identical_to_the_unfused_kernels_and_within_the_fp32_bound(dev, lib, shape):
    nf, hidden, e, cp, misaligned, pick = shape
    p = _inputs(dev, nf, hidden, e, cp, misaligned)
    assert _pick(lib, p) == pick
    ucoef, umod = p['unfused']
    ref = p['ref']
    table = torch.tensor(TABLE, device=dev)
    width = _width(p)
    for row in range(3):
        istep = torch.tensor([row], device=dev, dtype=torch.int64)
        coef, mod, out_step = _run(lib, dev, p, COS_VP, table=table, istep=istep)
        assert out_step.item() == row and istep.item() == row + 1
        assert _same_bits(coef.t[4:9], table[row, [2, 3, 4, 0, 1]])
        assert _same_bits(coef.t[0:4], ucoef[2 * row:2 * row + 2].reshape(-1)), 'mu / sigma vs sda_vp_schedule'
        assert _same_bits(mod.t.view(2, width), umod[2 * row:2 * row + 2]), 'mod vs sda_time_embed + sda_linear_small'
        assert torch.isnan(coef.t[9:16]).all(), 'out_coef[9:16] belongs to the tooling build'
        assert coef.guards_intact() and mod.guards_intact()
        sl = slice(2 * row, 2 * row + 2)
        _check_f64('prologue mu', coef.t[0:4:2], R.V(ref['mu'].v[sl], ref['mu'].e[sl]))
        _check_f64('prologue sigma', coef.t[1:4:2], R.V(ref['sigma'].v[sl], ref['sigma'].e[sl]))
        _check_f64('prologue mod', mod.t.view(2, width), R.V(ref['mod'].v[sl], ref['mod'].e[sl]))


@pytest.mark.parametrize('shape', SHAPES, ids=_IDS)
def test_prologue_t_dev_form_with_one_and_two_times(dev, lib, shape):
    nf, hidden, e, cp, misaligned, pick = shape
    p = _inputs(dev, nf, hidden, e, cp, misaligned)
    assert _pick(lib, p) == pick
    ucoef, umod = p['unfused']
    width = _width(p)
    for first in (0, 2, 4):
        t = torch.tensor(TIMES[first:first + 2], device=dev)
        for nt in (1, 2):
            coef, mod, out_step = _run(lib, dev, p, COS_VP, t=t, nt=nt)
            assert _same_bits(coef.t[0:2 * nt], ucoef[first:first + nt].reshape(-1))
            assert _same_bits(mod.t[:nt * width].view(nt, width), umod[first:first + nt])
            assert _same_bits(coef.t[7:7 + nt], t[:nt])
            assert out_step.item() == 0                                # (no table: step 0)
            assert torch.isnan(coef.t[4:7]).all() and torch.isnan(coef.t[9:16]).all()
            if nt == 1:
                assert torch.isnan(coef.t[2:4]).all() and torch.isnan(coef.t[8]) and torch.isnan(mod.t[width:]).all()
            assert coef.guards_intact() and mod.guards_intact()


def test_prologue_staged_and_misaligned_twin_agree_bit_for_bit(dev, lib):
    a = _inputs(dev, 16, 256, 32, 192, False)
    b = _inputs(dev, 16, 256, 32, 192, True)
    assert _pick(lib, a) == STAGED and _pick(lib, b) == UNSTAGED
    table = torch.tensor(TABLE, device=dev)
    for row in range(3):
        ra = _run(lib, dev, a, COS_VP, table=table, istep=torch.tensor([row], device=dev, dtype=torch.int64))
        rb = _run(lib, dev, b, COS_VP, table=table, istep=torch.tensor([row], device=dev, dtype=torch.int64))
        assert _same_bits(ra[0].t[:9], rb[0].t[:9]) and _same_bits(ra[1].t, rb[1].t)


@pytest.mark.parametrize('shape', [(16, 256, 32, 192, STAGED), (13, 100, 24, 7, UNSTAGED)], ids=['staged', 'unstaged'])
@pytest.mark.parametrize('sigma_kind', [0, 1, 2])
@pytest.mark.parametrize('alpha_kind', [0, 1, 2])
def test_prologue_schedules_are_sda_vp_schedule_bit_for_bit(dev, lib, shape, alpha_kind, sigma_kind):
    from sda_amd import ops
    nf, hidden, e, cp, pick = shape
    p = _inputs(dev, nf, hidden, e, cp, False)
    assert _pick(lib, p) == pick
    sched = (alpha_kind, ETA, STOCK_K[alpha_kind], sigma_kind)
    mu, sg = R.mu_sigma(np.float32(TIMES), *sched)
    for first in (0, 2, 4):
        t = torch.tensor(TIMES[first:first + 2], device=dev)
        coef, mod, _ = _run(lib, dev, p, sched, t=t, nt=2)
        want = torch.cat([ops.vp_schedule(t[i:i + 1], *sched) for i in range(2)])
        assert _same_bits(coef.t[0:4], want)
        assert _same_bits(mod.t.view(2, -1), p['unfused'][1][first:first + 2]), 'the schedule does not enter the embedding'
        sl = slice(first, first + 2)
        _check_f64('prologue mu', coef.t[0:4:2], R.V(mu.v[sl], mu.e[sl]))
        _check_f64('prologue sigma', coef.t[1:4:2], R.V(sg.v[sl], sg.e[sl]))


# ------------------------------------------------------------------------------------------------------------ keyed corrector
SEED = 0x1234567890abcdef
TAU = 0.25
# (row0, draw_dev, mul, add): the global row and the draw index draw_dev x mul + add on both sides of 2^32
KEYS = [(0, 11, 2, 1), (40, 3 * 2 ** 30, 2, 1), (2 ** 32 + 5, 11, 2, 1), (2 ** 32 + 5, 3 * 2 ** 30, 2, 1)]


def _keyed_case(dev, lib, b, per, nchunk, key, seed):
    """-> (x0, eps, partial, sigma, keyed result Guarded, unfused result)."""
    from sda_amd import _lib, ops
    row0, draw, mul, add = key
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(b, per, generator=g).to(dev)
    eps = torch.randn(b, per, generator=g).to(dev)
    partial = (torch.rand(b, nchunk, generator=g) * 50 + 1).to(dev)
    coef = torch.tensor([0.37], device=dev)
    draw_dev = torch.tensor([draw], device=dev, dtype=torch.int64)
    z = ops.randn_rows(torch.empty(b, per, device=dev), SEED, row0, draw_dev=draw_dev, draw_mul=mul, draw_add=add)
    want = x0.clone()
    ops.pc_correct(want, eps, z, b, partial, TAU, 0.0, coef_dev=coef, nchunk=nchunk)
    got = Guarded(b * per, dev, fill=x0)
    _lib.check(lib.sda_pc_correct_keyed(got.ptr(), eps.data_ptr(), b, per, partial.data_ptr(), nchunk, TAU, 0.0, coef.data_ptr(), SEED, row0,
                                        draw_dev.data_ptr(), mul, add, _stream()), 'sda_pc_correct_keyed')
    torch.cuda.synchronize()
    return x0, eps, partial, 0.37, got, want


@pytest.mark.parametrize('b,per', [(3, 1), (3, 2), (5, 7), (4, 64), (2, 4097), (6, 195)])
def test_keyed_corrector_is_randn_rows_plus_pc_correct_bit_for_bit(dev, lib, b, per):
    for nchunk in (1, 3):
        for i, key in enumerate(KEYS):
            x0, eps, partial, sigma, got, want = _keyed_case(dev, lib, b, per, nchunk, key, 10 * per + i)
            assert _same_bits(got.t.view(b, per), want), (nchunk, key)
            assert got.guards_intact()
            assert not torch.equal(want, x0)


def test_keyed_corrector_second_grid_stride_trip_with_a_ragged_last_quad(dev, lib):
    """2048 blocks x 256 threads x 4 elements = 2 097 152 per trip: 7 elements more take a second trip whose last quad holds 3"""
    b, per = 1, 2048 * 256 * 4 + 7
    for nchunk, key in ((3, KEYS[0]), (1, KEYS[3])):
        x0, eps, partial, sigma, got, want = _keyed_case(dev, lib, b, per, nchunk, key, 5)
        assert _same_bits(got.t.view(b, per), want)
        assert got.guards_intact()
        assert not torch.equal(want[:, -7:], x0[:, -7:])


@pytest.mark.parametrize('b,per', [(3, 1), (3, 2)])
def test_keyed_corrector_smallest_cases_against_float64(dev, lib, b, per):
    """z from the numpy Philox; tolerance: 2e-5 on the device normal (tests/test_gpu_parallel.py: fp32 log / sincos round-off) times its
    factor sqrt(2 delta) sigma, plus 4 u on the update's terms (one chunk: delta and sqrt(2 delta) carry 1 u each, then a product, the
    sum, the factor sigma and the subtraction)."""
    for i, key in enumerate(KEYS):
        row0, draw, mul, add = key
        x0, eps, partial, sigma, got, _ = _keyed_case(dev, lib, b, per, 1, key, 77 + i)
        z = philox_ref.randn_rows(b, per, SEED, row0, draw * mul + add).astype(np.float64)
        x, e = x0.double().cpu().numpy(), eps.double().cpu().numpy()
        sg = float(np.float32(sigma))
        delta = TAU / (partial.double().cpu().numpy().sum(axis=1, keepdims=True) / per)
        sq = np.sqrt(2 * delta)
        ref = x - (delta * e + sq * z) * sg
        tol = 2e-5 * sq * sg + 4 * U * (np.abs(x) + np.abs(delta * e * sg) + np.abs(sq * z * sg))
        err = np.abs(got.t.view(b, per).double().cpu().numpy() - ref)
        _note('pc_correct_keyed', (err / tol).max())
        assert (err <= tol).all(), key


# ------------------------------------------------------------------------------------------------------------ mc_finish
MC_CASES = [
    (3, 61, 2, 3),      # 15 values: 16-float rows
    (3, 11, 2, 4),      # 20 values: 32-float rows
    (2, 9, 0, 16),      # k = 0, exactly 16 values
    (2, 9, 0, 17),      # ... and the first size on 32-float rows
    (5, 1, 4, 3),       # one window
    (2, 120, 1, 3),     # 366 elements per trajectory: a thread's second trip
    (4, 2, 1, 2),       # 8 elements: less than a wavefront
    (1, 5, 0, 32),      # the widest window
]


def _mc_inputs(dev, b, nw, k, c):
    g = torch.Generator().manual_seed(b * 1000 + nw * 10 + k + c)
    L, wc = nw + 2 * k, (2 * k + 1) * c
    gld = 16 if wc <= 16 else 32
    eps, ghat, xs = (torch.randn(b, L, c, generator=g).to(dev) for _ in range(3))
    gwin = torch.full((b * nw, gld), float('nan'))
    gwin[:, :wc] = torch.randn(b * nw, wc, generator=g)               # the padding columns stay NaN: never read
    coef = torch.tensor([0.83, 0.55], device=dev)                      # mu, sigma
    step_coef = torch.tensor([0.97, 0.013], device=dev)                # r, c1
    return eps, ghat, xs, gwin.to(dev), coef, step_coef, gld


@pytest.mark.parametrize('affine', [False, True], ids=['bare', 'affine'])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('b,nw,k,c', MC_CASES)
def test_mc_finish_alone(dev, lib, b, nw, k, c, mode, affine):
    from sda_amd import _lib, ops
    eps, ghat, xs0, gwin, coef, step_coef, gld = _mc_inputs(dev, b, nw, k, c)
    L = nw + 2 * k
    per = L * c
    cx0, cx1 = (0.3, -0.2) if affine else (0.0, 0.0)
    out, xs, partial = Guarded(b * per, dev), Guarded(b * per, dev, fill=xs0), Guarded(b, dev)
    _lib.check(lib.sda_mc_finish(eps.data_ptr(), ghat.data_ptr(), gwin.data_ptr(), b, nw, k, c, cx0, cx1, coef.data_ptr(), mode, out.ptr(),
                                 xs.ptr(), step_coef.data_ptr(), partial.ptr(), _stream()), 'sda_mc_finish')
    torch.cuda.synchronize()
    assert out.guards_intact() and xs.guards_intact() and partial.guards_intact()
    if mode == 1:
        assert torch.isnan(out.t).all(), 'mode 1 writes x only'
    else:
        assert _same_bits(xs.t.view(b, L, c), xs0), 'modes 0 and 2 do not touch x'
    if mode != 2:
        assert torch.isnan(partial.t).all()
    res = xs.t if mode == 1 else out.t
    assert torch.isfinite(res).all(), 'a padding column of gwin was read'
    ref = R.mc_finish(eps.cpu().numpy(), ghat.cpu().numpy(), gwin.cpu().numpy(), nw, k, c, np.float32(cx0), np.float32(cx1), 0.83, 0.55, mode,
                      xs0.cpu().numpy(), step_coef.cpu().numpy())
    if not affine:
        # the unfused chain: overlap sum, guided combine, then the predictor / the sum of squares
        gx = torch.empty(b, L, c, device=dev)
        ops.unfold_adjoint(gwin, b, nw, k, c, 1, gld, gx)
        want = torch.empty(b, L, c, device=dev)
        ops.guided_combine(eps, ghat, gx, coef[0], coef[1], want)
        if mode == 1:
            x = xs0.clone()
            ops.pc_predict(x, want, 0.0, 0.0, coef_dev=step_coef)
            want = x
        assert _same_bits(res.view(b, L, c), want)
        if mode == 2:
            psum = torch.empty(b, ops.SUMSQ_CHUNKS, device=dev)
            assert ops.sumsq_partial(want, b, psum) == 1
            assert _same_bits(partial.t, psum.reshape(-1)[:b])
    # float64 (the affine estimator has no unfused kernel): 8 u on the magnitudes of the guided score's terms; mode 1: the predictor's two
    # products and sum on top
    tol = 8 * U * ref['mag']
    want64 = ref['out']
    if mode == 1:
        r, c1 = (float(v) for v in step_coef.double().cpu())
        tol = abs(c1) * tol + 2 * U * (np.abs(r * xs0.double().cpu().numpy()) + np.abs(c1 * want64))
        want64 = ref['x']
    err = np.abs(res.view(b, L, c).double().cpu().numpy() - want64)
    _note('mc_finish', (err / tol).max())
    assert (err <= tol).all()
    if mode == 2:
        # the sum of squares: ceil(per / 256) terms per thread, a six-level wave tree and two more levels across the four waves
        sumsq = (ref['out'] ** 2).reshape(b, -1).sum(axis=1)
        ptol = (math.ceil(per / 256) + 8) * U * sumsq
        perr = np.abs(partial.t.double().cpu().numpy() - ref['partial'])
        _note('mc_finish partial', (perr / ptol).max())
        assert (perr <= ptol).all()
