"""GPU: the 15 kernels of csrc/elementwise.hip and csrc/linear.hip, each alone, through the C ABI, against tests/glue_ref.py.

bit-exact class   pc_predict, denoise, guided_combine (with and without vjp), gauss_cotangent, pc_correct (on the device's own partial sums),
                  fold, fold_adjoint, unfold_adjoint: the bits of the float32 restatement; the coef_dev form the bits of the by-value form;
                  every one past its grid cap (the second grid-stride trip);
bounded class     linear (every NT instantiation, every boundary of the row / column / K tiles, every activation in all three places),
                  linear_small, row_ln, row_ln_bwd (both variance conventions, null and present statistics / residual), sumsq_partial (any
                  chunk count), time_embed, vp_schedule: within the float64 reference's derived fp32 bound.
Every output is a slice of a NaN-filled buffer with 64 floats of guard on each side; the guards must still be NaN afterwards.  Nothing is
skipped and no element is left out of a comparison."""
import numpy as np
import pytest
import torch

from tests import glue_cases as C
from tests import glue_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
#: worst error / bound per kernel of this run (printed: CHANGELOG.md quotes them)
RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))
    print(f'glue {what}: error / bound = {float(ratio):.3f} (worst so far {RATIOS[what]:.3f})')


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


class Guarded:
    """n floats between two NaN guard bands; prefilled with NaN unless `fill` is given."""

    def __init__(self, n, dev, fill=None):
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all()), 'a guard band was written'
        return self.t.cpu().numpy()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ok(rc, what):
    from sda_amd import _lib
    _lib.check(rc, what)


def _same_bits(got, want):
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _check(what, got, ref: 'R.V'):
    """every element within the bound (a bound of exactly 0 asks for the exact value)"""
    got = got.astype(np.float64).reshape(ref.v.shape)
    err = np.abs(got - ref.v)
    assert np.isfinite(got).all(), what
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / ref.e)
    _note(what.split(':')[0], ratio.max())
    assert (err <= ref.e).all(), f'{what}: {ratio.max():.3f} x the fp32 bound from float64'


# ------------------------------------------------------------------------------------------------------------ sda_linear
def _linear(lib, dev, x, w, b, out_f, trans_w=0, act_in=0, act_out=0, dact_z=None, act_d=0, res=None):
    rows, in_f = x.shape
    y = Guarded(rows * out_f, dev)
    _ok(lib.sda_linear(x.data_ptr(), rows, in_f, w.data_ptr(), _ptr(b), out_f, trans_w, act_in, act_out, _ptr(dact_z), act_d, _ptr(res),
                       y.ptr(), _stream()), 'sda_linear')
    return y.np()


@pytest.mark.parametrize('out_f', C.LIN_OUT)
def test_linear_plain_and_transposed_with_bias_at_every_tile_boundary(dev, lib, out_f):
    for rows, in_f, _ in C.lin_full(out_f):
        p = C.lin_inputs(rows, in_f, out_f)
        d = {k: v.to(dev) for k, v in p.items()}
        wt = p['w'].t().contiguous()
        wtd = wt.to(dev)
        plain = _linear(lib, dev, d['x'], d['w'], None, out_f)
        _check(f'linear: plain {rows}x{in_f}->{out_f}', plain, R.linear_64(p['x'], p['w']))
        tb = _linear(lib, dev, d['x'], wtd, d['b'], out_f, trans_w=1)
        _check(f'linear: trans_w + bias {rows}x{in_f}->{out_f}', tb, R.linear_64(p['x'], wt, p['b'], trans_w=True))
        # the same tile walk with another staging index: the two weight layouts agree bit for bit
        assert _same_bits(_linear(lib, dev, d['x'], wtd, None, out_f, trans_w=1), plain), (rows, in_f, out_f)
        assert _same_bits(_linear(lib, dev, d['x'], d['w'], d['b'], out_f), tb), (rows, in_f, out_f)


@pytest.mark.parametrize('a', C.ACTS, ids=[R.ACT_NAMES[a] for a in C.ACTS])
def test_linear_activation_in_the_loader_the_epilogue_and_as_a_derivative_with_residual(dev, lib, a):
    for rows, in_f, out_f in C.lin_thin():
        p = C.lin_inputs(rows, in_f, out_f)
        d = {k: v.to(dev) for k, v in p.items()}
        tag = f'{R.ACT_NAMES[a]} {rows}x{in_f}->{out_f}'
        _check(f'linear act_in: {tag}', _linear(lib, dev, d['x'], d['w'], d['b'], out_f, act_in=a), R.linear_64(p['x'], p['w'], p['b'], act_in=a))
        _check(f'linear act_out: {tag}', _linear(lib, dev, d['x'], d['w'], d['b'], out_f, act_out=a),
               R.linear_64(p['x'], p['w'], p['b'], act_out=a))
        _check(f'linear dact_z + res: {tag}', _linear(lib, dev, d['x'], d['w'], d['b'], out_f, dact_z=d['z'], act_d=a, res=d['res']),
               R.linear_64(p['x'], p['w'], p['b'], dact_z=p['z'], act_d=a, res=p['res']))


def test_linear_all_three_activation_sites_at_once_and_the_identity_derivative(dev, lib):
    rows, in_f, out_f = 129, 17, 65
    p = C.lin_inputs(rows, in_f, out_f)
    d = {k: v.to(dev) for k, v in p.items()}
    got = _linear(lib, dev, d['x'], d['w'], d['b'], out_f, act_in=R.GELU, act_out=R.ELU, dact_z=d['z'], act_d=R.SELU, res=d['res'])
    _check('linear: three sites', got, R.linear_64(p['x'], p['w'], p['b'], act_in=R.GELU, act_out=R.ELU, dact_z=p['z'], act_d=R.SELU, res=p['res']))
    # act_d = 0 multiplies by exactly 1
    assert _same_bits(_linear(lib, dev, d['x'], d['w'], d['b'], out_f, dact_z=d['z'], act_d=0), _linear(lib, dev, d['x'], d['w'], d['b'], out_f))


# ------------------------------------------------------------------------------------------------------------ row LayerNorm
def _row_ln(lib, dev, x, unbiased, stats):
    rows, f = x.shape
    y = Guarded(rows * f, dev)
    mean, rstd = (Guarded(rows, dev), Guarded(rows, dev)) if stats else (None, None)
    _ok(lib.sda_row_ln(x.data_ptr(), rows, f, C.LN_EPS, int(unbiased), y.ptr(), mean.ptr() if stats else None, rstd.ptr() if stats else None,
                       _stream()), 'sda_row_ln')
    return y.np(), (mean.np() if stats else None), (rstd.np() if stats else None)


def _row_ln_case(lib, dev, rows, f, unbiased, offset):
    p = C.ln_inputs(rows, f, offset)
    xd, gd, rd = (p[k].to(dev) for k in ('x', 'g', 'res'))
    y64, m64, r64 = R.row_ln_64(p['x'], C.LN_EPS, unbiased)
    tag = f'{rows}x{f} unbiased={unbiased} offset={offset}'
    y, mean, rstd = _row_ln(lib, dev, xd, unbiased, True)
    _check(f'row_ln: {tag}', y, y64)
    _check(f'row_ln mean: {tag}', mean, m64)
    _check(f'row_ln rstd: {tag}', rstd, r64)
    y0, _, _ = _row_ln(lib, dev, xd, unbiased, False)
    assert _same_bits(y0, y), 'the statistics outputs do not enter y'
    # backward on statistics of its own: the float64 ones rounded to fp32 (not the forward kernel's)
    m32, r32 = torch.from_numpy(m64.v.astype(np.float32)), torch.from_numpy(r64.v.astype(np.float32))
    md, sd = m32.to(dev), r32.to(dev)
    for res, resd in ((None, None), (p['res'], rd)):
        gx = Guarded(rows * f, dev)
        _ok(lib.sda_row_ln_bwd(gd.data_ptr(), xd.data_ptr(), rows, f, md.data_ptr(), sd.data_ptr(), int(unbiased), _ptr(resd), gx.ptr(),
                               _stream()), 'sda_row_ln_bwd')
        _check(f'row_ln_bwd: {tag} res={res is not None}', gx.np(), R.row_ln_bwd_64(p['g'], p['x'], m32, r32, unbiased, res))


@pytest.mark.parametrize('f', C.LN_F)
def test_row_ln_and_its_backward_at_every_register_and_workgroup_tail(dev, lib, f):
    for rows, ff, unbiased in C.ln_cases():
        if ff == f:
            _row_ln_case(lib, dev, rows, f, unbiased, False)


@pytest.mark.parametrize('unbiased', [False, True])
def test_row_ln_on_rows_whose_mean_dwarfs_their_spread(dev, lib, unbiased):
    _row_ln_case(lib, dev, *C.LN_OFFSET, unbiased, True)


# ------------------------------------------------------------------------------------------------------------ fold family
def _fold_all(lib, dev, b, nw, k, c, hw, extras, which=('fold', 'fold_adjoint', 'unfold_adjoint')):
    L, wl = nw + 2 * k, 2 * k + 1
    for extra in extras:
        p = C.fold_inputs(b, nw, k, c, hw, extra)
        if 'fold' in which and extra == extras[0]:
            out = Guarded(b * L * c * hw, dev)
            sd = p['s'].to(dev)
            _ok(lib.sda_fold(sd.data_ptr(), b, nw, k, c, hw, out.ptr(), _stream()), 'sda_fold')
            assert _same_bits(out.np(), R.fold_32(p['s'].numpy(), k, c)), ('fold', b, nw, k, c, hw)
        if 'fold_adjoint' in which and extra == extras[0]:
            gs = Guarded(b * nw * wl * c * hw, dev)
            gd = p['g'].to(dev)
            _ok(lib.sda_fold_adjoint(gd.data_ptr(), b, nw, k, c, hw, gs.ptr(), _stream()), 'sda_fold_adjoint')
            assert _same_bits(gs.np(), R.fold_adjoint_32(p['g'].numpy(), nw, k)), ('fold_adjoint', b, nw, k, c, hw)
        if 'unfold_adjoint' in which:
            gx = Guarded(b * L * c * hw, dev)
            wd = p['gwin'].to(dev)
            _ok(lib.sda_unfold_adjoint(wd.data_ptr(), b, nw, k, c, hw, wl * c + extra, gx.ptr(), _stream()), 'sda_unfold_adjoint')
            got = gx.np()
            assert np.isfinite(got).all(), 'a channel past (2k+1) c was read'
            assert _same_bits(got, R.unfold_adjoint_32(p['gwin'].numpy(), k, c)), ('unfold_adjoint', b, nw, k, c, hw, extra)


@pytest.mark.parametrize('b,nw,k,c,hw', C.fold_cases())
def test_fold_family_bit_for_bit_with_context_channel_strides(dev, lib, b, nw, k, c, hw):
    _fold_all(lib, dev, b, nw, k, c, hw, C.FOLD_EXTRA)


@pytest.mark.parametrize('which', ['fold', 'fold_adjoint', 'unfold_adjoint'])
def test_fold_family_three_elements_past_the_grid_cap(dev, lib, which):
    _fold_all(lib, dev, *C.FOLD_BIG[which], (0,), which=(which,))


# ------------------------------------------------------------------------------------------------------------ PC / guidance
@pytest.mark.parametrize('numel', C.PC_NUMEL)
def test_predictor_and_guidance_glue_bit_for_bit_in_both_call_forms(dev, lib, numel):
    x, eps, z = C.pc_inputs(numel)
    xd, ed, zd = x.to(dev), eps.to(dev), z.to(dev)
    step = torch.tensor([C.R, C.C1], device=dev)
    coef = torch.tensor([C.MU, C.SIGMA], device=dev)
    s = _stream()

    def both(what, launch, want, fill=None):
        """by-value arguments, then the device pair with poisoned by-value ones"""
        for form in (0, 1):
            out = Guarded(numel, dev, fill=fill)
            _ok(launch(out.ptr(), form), what)
            assert _same_bits(out.np(), want), (what, 'coef_dev' if form else 'by value')

    both('sda_pc_predict', lambda o, f: lib.sda_pc_predict(o, ed.data_ptr(), numel, 7.0 if f else C.R, 7.0 if f else C.C1, _ptr(step) if f else None, s),
         R.pc_predict_32(x, eps, C.R, C.C1), fill=xd)
    both('sda_denoise', lambda o, f: lib.sda_denoise(xd.data_ptr(), ed.data_ptr(), numel, 7.0 if f else C.MU, 7.0 if f else C.SIGMA,
                                                     _ptr(coef) if f else None, o, s), R.denoise_32(x, eps, C.MU, C.SIGMA))
    for vjp, vd in ((x, xd), (None, None)):
        both('sda_guided_combine', lambda o, f: lib.sda_guided_combine(ed.data_ptr(), zd.data_ptr(), _ptr(vd), numel, 7.0 if f else C.MU,
                                                                       7.0 if f else C.SIGMA, _ptr(coef) if f else None, o, s),
             R.guided_combine_32(eps, z, vjp, C.MU, C.SIGMA))
    # y per element, then y shared over a leading axis of the smallest size that divides (the cap case: 2 097 157 = 53 x 39 569)
    for y_numel in sorted({numel, numel // _smallest_divisor(numel)}):
        yd = zd[:y_numel].contiguous()
        both('sda_gauss_cotangent', lambda o, f: lib.sda_gauss_cotangent(yd.data_ptr(), y_numel, xd.data_ptr(), numel, C.STD, C.GAMMA,
                                                                         7.0 if f else C.MU, 7.0 if f else C.SIGMA, _ptr(coef) if f else None, o, s),
             R.gauss_cotangent_32(z[:y_numel], x, C.STD, C.GAMMA, C.MU, C.SIGMA))


def _smallest_divisor(n):
    return next((d for d in range(2, 1000) if n % d == 0), 1)


def test_the_cap_case_of_gauss_cotangent_has_a_broadcast_y():
    assert _smallest_divisor(C.PC_CAP + 5) == 53 and _smallest_divisor(255) == 3 and _smallest_divisor(257) == 257


@pytest.mark.parametrize('b', C.CORRECT_B)
@pytest.mark.parametrize('per', C.CORRECT_PER)
def test_corrector_bit_for_bit_on_the_device_partial_sums(dev, lib, per, b):
    from sda_amd import ops
    x, eps, z = (t.reshape(b, per) for t in C.pc_inputs(b * per, seed=b))
    xd, ed, zd = x.to(dev), eps.to(dev), z.to(dev)
    sig = torch.tensor([C.SIGMA], device=dev)
    for nchunk in sorted({ops.sumsq_chunks(per), 7}):
        partial = Guarded(b * nchunk, dev)
        _ok(lib.sda_sumsq_partial(ed.data_ptr(), b, per, partial.ptr(), nchunk, _stream()), 'sda_sumsq_partial')
        pn = partial.np().reshape(b, nchunk)
        want = R.pc_correct_32(x, eps, z, pn, C.TAU, C.SIGMA)
        for form in (0, 1):
            out = Guarded(b * per, dev, fill=xd)
            _ok(lib.sda_pc_correct(out.ptr(), ed.data_ptr(), zd.data_ptr(), b, per, partial.ptr(), nchunk, C.TAU, 7.0 if form else C.SIGMA,
                                   _ptr(sig) if form else None, _stream()), 'sda_pc_correct')
            assert _same_bits(out.np(), want), (per, b, nchunk, 'coef_dev' if form else 'by value')
        # and the step is the reference's within the float64 bound of the whole chain
        ss = R.sumsq_64(eps)
        _check(f'sumsq_partial: total {b}x{per}/{nchunk}', pn.astype(np.float64).sum(1), ss)


@pytest.mark.parametrize('per', C.SUMSQ_PER)
def test_sumsq_partial_at_any_chunk_count(dev, lib, per):
    b = 3
    eps = C.pc_inputs(b * per)[1].reshape(b, per)
    ed = eps.to(dev)
    total = R.sumsq_64(eps)
    for nchunk in C.SUMSQ_NCHUNK:
        partial = Guarded(b * nchunk, dev)
        _ok(lib.sda_sumsq_partial(ed.data_ptr(), b, per, partial.ptr(), nchunk, _stream()), 'sda_sumsq_partial')
        pn = partial.np().reshape(b, nchunk)
        chunk = -(-per // nchunk)
        for j in range(nchunk):
            if j * chunk >= per:
                assert (pn[:, j].view(np.int32) == 0).all(), f'empty trailing chunk {j} of {nchunk} is not +0.0'
        full = [j for j in range(nchunk) if j * chunk < per]
        for j in (full[0], full[len(full) // 2], full[-1]):
            _check(f'sumsq_partial: chunk {j}/{nchunk} of {per}', pn[:, j], R.sumsq_64(eps[:, j * chunk:(j + 1) * chunk]))
        _check(f'sumsq_partial: sum of {nchunk} chunks of {per}', pn.astype(np.float64).sum(1), total)


# ------------------------------------------------------------------------------------------------------------ time embedding / projection
@pytest.mark.parametrize('nt', C.TE_NT)
@pytest.mark.parametrize('nf,hidden,e', C.TE_SHAPES)
def test_time_embed_within_the_fp32_bound(dev, lib, nf, hidden, e, nt):
    p = C.te_inputs(nf, hidden, e, nt)
    d = {k: v.to(dev) for k, v in p.items()}
    emb = Guarded(nt * e, dev)
    _ok(lib.sda_time_embed(d['t'].data_ptr(), nt, d['freqs'].data_ptr(), nf, d['w0'].data_ptr(), d['b0'].data_ptr(), hidden, d['w2'].data_ptr(),
                           d['b2'].data_ptr(), e, emb.ptr(), _stream()), 'sda_time_embed')
    _check(f'time_embed: {nf}-{hidden}-{e} nt={nt}', emb.np(), R.time_embed_64(p['t'], p['freqs'], p['w0'], p['b0'], p['w2'], p['b2']))


@pytest.mark.parametrize('in_f', C.LS_IN)
def test_linear_small_ragged_last_workgroup_and_null_bias(dev, lib, in_f):
    for rows, out_f in C.LS_ROWS_OUT:
        p = C.ls_inputs(rows, in_f, out_f)
        d = {k: v.to(dev) for k, v in p.items()}
        for b, bd in ((None, None), (p['b'], d['b'])):
            y = Guarded(rows * out_f, dev)
            _ok(lib.sda_linear_small(d['x'].data_ptr(), rows, in_f, d['w'].data_ptr(), _ptr(bd), out_f, y.ptr(), _stream()), 'sda_linear_small')
            _check(f'linear_small: {rows}x{in_f}->{out_f} bias={b is not None}', y.np(), R.linear_small_64(p['x'], p['w'], b))


@pytest.mark.parametrize('sigma_kind', [0, 1, 2])
@pytest.mark.parametrize('alpha_kind', [0, 1, 2])
def test_vp_schedule_within_the_fp32_bound(dev, lib, alpha_kind, sigma_kind):
    t = np.asarray(C.VP_T, dtype=np.float32)
    mu, sg = R.mu_sigma(t, alpha_kind, C.ETA, C.VP_K[alpha_kind], sigma_kind)
    for i, tv in enumerate(t):
        td = torch.tensor([tv], device=dev)
        out = Guarded(2, dev)
        _ok(lib.sda_vp_schedule(td.data_ptr(), alpha_kind, C.ETA, C.VP_K[alpha_kind], sigma_kind, out.ptr(), _stream()), 'sda_vp_schedule')
        got = out.np()
        _check(f'vp_schedule mu: {alpha_kind}/{sigma_kind} t={tv}', got[0:1], R.V(mu.v[i:i + 1], mu.e[i:i + 1]))
        _check(f'vp_schedule sigma: {alpha_kind}/{sigma_kind} t={tv}', got[1:2], R.V(sg.v[i:i + 1], sg.e[i:i + 1]))
