"""CPU: tests/glue_ref.py against what the project already trusts (oracle.sda_oracle's fold / unfold / layer_norm / time_embedding / Schedule
and torch float64 F.linear / autograd) at the shapes tests/test_gpu_glue.py uses, every float32 restatement inside its float64 bound, and
every SDA_E_BADARG / SDA_E_UNSUPPORTED return of the 15 launchers of csrc/elementwise.hip and csrc/linear.hip (each returns before anything
is launched; no address is ever read)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sda_oracle as O
from tests import glue_cases as C
from tests import glue_ref as R

BADARG, UNSUPPORTED = -1, -2
PTR = 1 << 20               # a non-null address that is never dereferenced
ACT_NAME = {1: 'SiLU', 2: 'ReLU', 3: 'ELU', 4: 'GELU', 5: 'SELU'}


def _close64(got, want, n=8, mag=None):
    """two float64 evaluations of one formula"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    mag = np.abs(want) if mag is None else mag
    assert got.shape == want.shape
    assert (np.abs(got - want) <= R.f64_tol(n, mag)).all(), float(np.abs(got - want).max())


def _close_v(ref: 'R.V', want):
    """a float64 restatement of the formula ref.v evaluates: within the fp32 bound rescaled to float64's unit round-off (2^-53 / 2^-24),
    four times over (both sides round)"""
    want = np.asarray(want, dtype=np.float64)
    assert ref.v.shape == want.shape
    assert (np.abs(ref.v - want) <= ref.e * 2.0 ** -27).all(), float(np.abs(ref.v - want).max())


def _inside(f32_value, ref: 'R.V'):
    err = np.abs(np.asarray(f32_value, dtype=np.float64) - ref.v)
    assert (err <= ref.e).all(), float((err / np.maximum(ref.e, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize('a', C.ACTS)
def test_activations_and_derivatives_are_torch_float64(a):
    v = torch.linspace(-R.ACT_RANGE, R.ACT_RANGE, 4801, dtype=torch.float64)
    vv = v.clone().requires_grad_(True)
    y = O.activation(ACT_NAME[a])(vv)
    d, = torch.autograd.grad(y.sum(), vv)
    val, der, mag = R.act_terms(a, v.numpy())
    _close64(val, y.detach().numpy(), mag=mag + 1e-300)
    _close64(der, d.numpy(), mag=R.dact_terms(a, v.numpy())[1] + 1e-300)
    _close64(R.dact_terms(a, v.numpy())[0], d.numpy(), mag=R.dact_terms(a, v.numpy())[1] + 1e-300)
    assert (mag >= np.abs(val)).all() and (R.dact_terms(a, v.numpy())[1] >= np.abs(der) * (1 - 1e-15)).all()


def test_every_allowance_is_twice_its_measured_value():
    assert set(R.ALLOW) == set(R.MEASURED)
    for key, m in R.MEASURED.items():
        assert m > 0 and 2 * m <= R.ALLOW[key] <= 2 * m + 0.01, key


# ------------------------------------------------------------------------------------------------ sda_linear
@pytest.mark.parametrize('out_f', C.LIN_OUT)
def test_linear_reference_is_f_linear_in_float64(out_f):
    for rows, in_f, _ in C.lin_full(out_f):
        p = C.lin_inputs(rows, in_f, out_f)
        x, w, b = p['x'].double(), p['w'].double(), p['b'].double()
        mag = (x.abs() @ w.abs().T + b.abs()).numpy()
        _close64(R.linear_64(p['x'], p['w'], None).v, F.linear(x, w).numpy(), in_f, mag)
        ref = R.linear_64(p['x'], p['w'].t().contiguous(), p['b'], trans_w=True)
        _close64(ref.v, F.linear(x, w, b).numpy(), in_f, mag)
        assert (ref.e >= U_(in_f) * mag * 0.999).all()
        # the plain float32 evaluation lies inside the bound
        _inside(F.linear(p['x'], p['w'], p['b']).numpy(), R.linear_64(p['x'], p['w'], p['b']))


def U_(n):
    return (n + 2) * R.U


@pytest.mark.parametrize('a', C.ACTS)
def test_linear_reference_with_activations_is_torch_autograd_in_float64(a):
    act = O.activation(ACT_NAME[a])
    for rows, in_f, out_f in C.lin_thin():
        p = C.lin_inputs(rows, in_f, out_f)
        x, w, b, res = p['x'].double(), p['w'].double(), p['b'].double(), p['res'].double()
        mag = (act(x).abs() @ w.abs().T + b.abs()).numpy() + 1e-300
        _close64(R.linear_64(p['x'], p['w'], p['b'], act_in=a).v, F.linear(act(x), w, b).numpy(), in_f, mag)
        pre = F.linear(x, w, b)
        mag = (x.abs() @ w.abs().T + b.abs()).numpy() * 2
        _close64(R.linear_64(p['x'], p['w'], p['b'], act_out=a).v, act(pre).numpy(), in_f, mag)
        z = p['z'].double().requires_grad_(True)
        dz, = torch.autograd.grad(act(z).sum(), z)
        ref = R.linear_64(p['x'], p['w'], p['b'], dact_z=p['z'], act_d=a, res=p['res'])
        _close64(ref.v, (pre * dz + res).numpy(), in_f, mag * 2 + res.abs().numpy())
        # float32 torch lies inside the bound (its own activation error is not the device's: only the exact ones)
        if a == 2:
            _inside((F.linear(p['x'], p['w'], p['b']) * dz.float() + p['res']).numpy(), ref)


# ------------------------------------------------------------------------------------------------ row LayerNorm
@pytest.mark.parametrize('rows,f,unbiased', C.ln_cases())
def test_row_ln_reference_is_the_oracle_layer_norm_and_its_autograd(rows, f, unbiased):
    for offset in ((False, True) if (rows, f) == C.LN_OFFSET else (False,)):
        p = C.ln_inputs(rows, f, offset)
        x = p['x'].double().requires_grad_(True)
        want = O.layer_norm(x, dim=-1, eps=float(np.float32(C.LN_EPS)), unbiased=unbiased)
        y, mean, rstd = R.row_ln_64(p['x'], C.LN_EPS, unbiased)
        _close_v(y, want.detach().numpy())
        _close_v(mean, x.detach().mean(1).numpy())
        # the float32 restatement in the kernel's order of formulas (sequential sums) lies inside the bound
        x32 = p['x'].numpy()
        m32 = (x32.sum(1, dtype=np.float32) / np.float32(f))[:, None]
        d32 = x32 - m32
        r32 = np.float32(1.0) / np.sqrt((d32 * d32).sum(1, dtype=np.float32)[:, None] / np.float32(f - 1 if unbiased else f) + np.float32(C.LN_EPS))
        assert (d32 * r32).dtype == np.float32
        _inside(d32 * r32, y)
        _inside(m32[:, 0], mean)
        _inside(r32[:, 0], rstd)
        # backward on the float32 statistics it is given
        m_t, r_t = torch.from_numpy(m32[:, 0].copy()), torch.from_numpy(r32[:, 0].copy())
        for res in (None, p['res']):
            ref = R.row_ln_bwd_64(p['g'], p['x'], m_t, r_t, unbiased, res)
            # autograd through the same formula with the GIVEN statistics' float64 values: h = (x - m) r, and the backward of
            # standardisation written out (what the kernel implements)
            g = p['g'].double()
            h = (x.detach() - m_t.double()[:, None]) * r_t.double()[:, None]
            gx = r_t.double()[:, None] * (g - g.mean(1, keepdim=True) - h * (g * h).sum(1, keepdim=True) / (f - 1 if unbiased else f))
            if res is not None:
                gx = gx + res.double()
            _close_v(ref, gx.numpy())
            assert (ref.e >= 0).all()
        if not offset:
            # with statistics of full precision the written-out backward IS autograd through the oracle
            gref, = torch.autograd.grad(want, x, p['g'].double())
            xd = x.detach()
            m64 = xd.mean(1)
            r64 = 1.0 / torch.sqrt(((xd - m64[:, None]) ** 2).sum(1) / (f - 1 if unbiased else f) + float(np.float32(C.LN_EPS)))
            _close_v(R.row_ln_bwd_64(p['g'], p['x'], m64.numpy(), r64.numpy(), unbiased, None, exact_stats=True), gref.numpy())


# ------------------------------------------------------------------------------------------------ fold family
@pytest.mark.parametrize('b,nw,k,c,hw', C.fold_cases())
def test_fold_references_are_the_oracle_and_its_autograd(b, nw, k, c, hw):
    for extra in C.FOLD_EXTRA:
        p = C.fold_inputs(b, nw, k, c, hw, extra)
        wl, L = 2 * k + 1, nw + 2 * k
        s = p['s'].reshape(b, nw, wl * c, hw, 1).double().requires_grad_(True)
        ref = O.fold(s, k)
        assert np.array_equal(R.fold_32(p['s'].numpy(), k, c), ref.detach().float().numpy()[..., 0])
        gs, = torch.autograd.grad(ref, s, p['g'].double().reshape(b, L, c, hw, 1))
        assert np.array_equal(R.fold_adjoint_32(p['g'].numpy(), nw, k).reshape(b, nw, wl * c, hw), gs.float().numpy()[..., 0])
        x = torch.zeros(b, L, c, hw, dtype=torch.float64, requires_grad=True)
        gw = p['gwin'][:, :, :wl * c]
        gx, = torch.autograd.grad(O.unfold(x, k), x, gw.double())
        r64 = R.unfold_adjoint_64(p['gwin'].numpy(), k, c)
        _close_v(r64, gx.numpy())
        r32 = R.unfold_adjoint_32(p['gwin'].numpy(), k, c)
        assert r32.dtype == np.float32 and np.isfinite(r32).all()
        _inside(r32, r64)


def test_big_fold_shapes_are_three_elements_past_the_grid_cap():
    b, nw, k, c, hw = C.FOLD_BIG['fold']
    assert b * (nw + 2 * k) * c * hw == C.FOLD_CAP + 3
    b, nw, k, c, hw = C.FOLD_BIG['fold_adjoint']
    assert b * nw * (2 * k + 1) * c * hw == C.FOLD_CAP + 3
    b, nw, k, c, hw = C.FOLD_BIG['unfold_adjoint']
    assert b * (nw + 2 * k) * c * hw == C.FOLD_CAP + 3


# ------------------------------------------------------------------------------------------------ PC / guidance
@pytest.mark.parametrize('numel', C.PC_NUMEL[:4] + (4099,))
def test_pc_and_guidance_float32_restatements_lie_inside_their_float64_bounds(numel):
    x, eps, z = C.pc_inputs(numel)
    _inside(R.pc_predict_32(x, eps, C.R, C.C1), R.pc_predict_64(x, eps, C.R, C.C1))
    _inside(R.denoise_32(x, eps, C.MU, C.SIGMA), R.denoise_64(x, eps, C.MU, C.SIGMA))
    _inside(R.guided_combine_32(eps, z, x, C.MU, C.SIGMA), R.guided_combine_64(eps, z, x, C.MU, C.SIGMA))
    _inside(R.guided_combine_32(eps, z, None, C.MU, C.SIGMA), R.guided_combine_64(eps, z, None, C.MU, C.SIGMA))
    _inside(R.gauss_cotangent_32(z, x, C.STD, C.GAMMA, C.MU, C.SIGMA), R.gauss_cotangent_64(z, x, C.STD, C.GAMMA, C.MU, C.SIGMA))
    # the float64 values are the reference's expressions (sda/score.py:250-261, 387-396)
    X, E, Z = x.double().numpy(), eps.double().numpy(), z.double().numpy()
    mu, sg, r, c1, std, gam = (float(np.float32(v)) for v in (C.MU, C.SIGMA, C.R, C.C1, C.STD, C.GAMMA))
    _close64(R.pc_predict_64(x, eps, C.R, C.C1).v, r * X + c1 * E, mag=np.abs(r * X) + np.abs(c1 * E))
    _close64(R.denoise_64(x, eps, C.MU, C.SIGMA).v, (X - sg * E) / mu, mag=(np.abs(X) + np.abs(sg * E)) / mu)
    _close64(R.guided_combine_64(eps, z, x, C.MU, C.SIGMA).v, E - sg * (Z / mu - (sg / mu) * X), mag=np.abs(E) + np.abs(Z) + np.abs(X))
    _close64(R.guided_combine_64(eps, z, None, C.MU, C.SIGMA).v, E - sg * (Z / mu), mag=np.abs(E) + np.abs(Z))
    _close64(R.gauss_cotangent_64(z, x, C.STD, C.GAMMA, C.MU, C.SIGMA).v, (Z - X) / (std ** 2 + gam * (sg / mu) ** 2), mag=(np.abs(Z) + np.abs(X)) * 8)


def test_gauss_cotangent_broadcasts_y_over_the_leading_axis():
    x, eps, z = C.pc_inputs(35)
    got = R.gauss_cotangent_32(z[:7], x.reshape(5, 7), C.STD, C.GAMMA, C.MU, C.SIGMA)
    want = R.gauss_cotangent_32(z[:7].repeat(5), x, C.STD, C.GAMMA, C.MU, C.SIGMA)
    assert np.array_equal(got.reshape(-1), want)


@pytest.mark.parametrize('b', C.CORRECT_B)
@pytest.mark.parametrize('per', C.CORRECT_PER[:2])
def test_corrector_restatement_lies_inside_its_bound_and_is_the_reference_step(b, per):
    x, eps, z = (t.reshape(b, per) for t in C.pc_inputs(b * per))
    for nchunk in (1, 7):
        chunk = -(-per // nchunk)
        e32 = eps.numpy()
        partial = np.stack([(e32[:, j * chunk:(j + 1) * chunk] ** 2).sum(1, dtype=np.float32) for j in range(nchunk)], axis=1)
        ref = R.pc_correct_64(x, eps, z, partial, C.TAU, C.SIGMA)
        _inside(R.pc_correct_32(x, eps, z, partial, C.TAU, C.SIGMA), ref)
        # score.py:257-261 with the exact mean of eps^2: within the bound plus what the partial sums' own rounding moves delta by
        ss = R.sumsq_64(eps)
        _inside(partial.astype(np.float64).sum(1), ss)
        E = eps.double().numpy()
        delta = float(np.float32(C.TAU)) / (E ** 2).mean(1, keepdims=True)
        want = x.double().numpy() - (delta * E + np.sqrt(2 * delta) * z.double().numpy()) * float(np.float32(C.SIGMA))
        rel = (ss.e / ss.v)[:, None]
        slack = rel * (np.abs(delta * E) + np.abs(np.sqrt(2 * delta) * z.double().numpy())) * 2
        assert (np.abs(ref.v - want) <= ref.e + slack).all()


@pytest.mark.parametrize('per', C.SUMSQ_PER)
def test_sumsq_bound_holds_for_sequential_pairwise_and_chunked_float32_sums(per):
    eps = C.pc_inputs(3 * per)[1].reshape(3, per)
    ref = R.sumsq_64(eps)
    e32 = eps.numpy()
    seq = np.zeros(3, dtype=np.float32)
    for i in range(0, per, max(1, per // 997)):
        seq = seq + (e32[:, i:i + max(1, per // 997)] ** 2).sum(1, dtype=np.float32)
    _inside(seq, ref)
    _inside(np.cumsum(e32 ** 2, axis=1, dtype=np.float32)[:, -1], ref)          # one sequential chain of `per` additions
    _close64(ref.v, (eps.double() ** 2).sum(1).numpy(), per)


# ------------------------------------------------------------------------------------------------ time embedding / projection
@pytest.mark.parametrize('nt', C.TE_NT)
@pytest.mark.parametrize('nf,hidden,e', C.TE_SHAPES)
def test_time_embed_reference_is_the_oracle_in_float64(nf, hidden, e, nt):
    p = C.te_inputs(nf, hidden, e, nt)
    sd = {'e.freqs': p['freqs'].double(), 'e.0.weight': p['w0'].double(), 'e.0.bias': p['b0'].double(), 'e.2.weight': p['w2'].double(),
          'e.2.bias': p['b2'].double()}
    want = O.time_embedding(sd, 'e.', p['t'].double())
    ref = R.time_embed_64(p['t'], p['freqs'], p['w0'], p['b0'], p['w2'], p['b2'])
    assert ref.v.shape == (nt, e) and (ref.e > 0).all()
    _close64(ref.v, want.numpy(), hidden + 2 * nf, mag=np.abs(ref.v) + 1.0)
    got32 = O.time_embedding({k: v.float() for k, v in sd.items()}, 'e.', p['t'])
    _inside(got32.numpy(), ref)


@pytest.mark.parametrize('rows,out_f', C.LS_ROWS_OUT)
@pytest.mark.parametrize('in_f', C.LS_IN)
def test_linear_small_reference_is_f_linear_in_float64(rows, out_f, in_f):
    p = C.ls_inputs(rows, in_f, out_f)
    for b in (None, p['b']):
        ref = R.linear_small_64(p['x'], p['w'], b)
        want = F.linear(p['x'].double(), p['w'].double(), None if b is None else b.double())
        _close64(ref.v, want.numpy(), in_f, mag=(p['x'].double().abs() @ p['w'].double().abs().T).numpy() + 1.0)
        _inside(F.linear(p['x'], p['w'], b).numpy(), ref)


@pytest.mark.parametrize('sigma_kind,kind', enumerate(('vp', 'subvp', 'subsubvp')))
@pytest.mark.parametrize('alpha_kind,alpha', enumerate(('lin', 'cos', 'exp')))
def test_schedule_reference_is_the_oracle_schedule(alpha_kind, alpha, sigma_kind, kind):
    t = np.asarray(C.VP_T, dtype=np.float32)
    eta = float(np.float32(C.ETA))
    k = (0.0, math.acos(math.sqrt(eta)), math.log(eta))[alpha_kind]
    sched = O.Schedule(alpha, eta=eta, kind=kind)
    tt = torch.from_numpy(t.astype(np.float64))
    mu, sg = R.vp_64(t, alpha_kind, eta, k, sigma_kind)
    _close64(mu, sched.mu(tt).numpy(), mag=1.0)
    _close64(sg, sched.sigma(tt).numpy(), mag=np.maximum(1.0, 1.0 / np.maximum(sg, 1e-3)))
    # the bounded form evaluates the same formula on the fp32 eta and k the kernel receives
    k32 = float(np.float32(C.VP_K[alpha_kind]))
    bmu, bsg = R.mu_sigma(t, alpha_kind, C.ETA, C.VP_K[alpha_kind], sigma_kind)
    mu32, sg32 = R.vp_64(t, alpha_kind, eta, k32, sigma_kind)
    _close64(bmu.v, mu32, mag=1.0)
    _close64(bsg.v, sg32, mag=np.maximum(1.0, 1.0 / np.maximum(sg32, 1e-3)))
    assert (bmu.e >= 0).all() and (bsg.e > 0).all()


# ------------------------------------------------------------------------------------------------ argument checks (no launch)
@pytest.fixture(scope='module')
def lib():
    from sda_amd import _lib
    return _lib.load()


def _each_null(call, names):
    for name in names:
        assert call(**{name: None}) == BADARG, name


def test_time_embed_argument_checks(lib):
    def call(t=PTR, nt=2, freqs=PTR, nf=16, w0=PTR, b0=PTR, hidden=256, w2=PTR, b2=PTR, e=32, emb=PTR):
        return lib.sda_time_embed(t, nt, freqs, nf, w0, b0, hidden, w2, b2, e, emb, None)
    _each_null(call, ('t', 'freqs', 'w0', 'b0', 'w2', 'b2', 'emb'))
    for name in ('nt', 'nf', 'hidden', 'e'):
        assert call(**{name: 0}) == BADARG and call(**{name: -1}) == BADARG, name
    assert call(nf=65) == UNSUPPORTED                      # 2 nf = 130 features: one pair past the LDS row
    assert call(hidden=1025) == UNSUPPORTED
    assert call(nf=65, emb=None) == BADARG                 # a bad argument wins


def test_linear_small_argument_checks(lib):
    def call(x=PTR, rows=7, in_f=64, w=PTR, b=PTR, out_f=300, y=PTR):
        return lib.sda_linear_small(x, rows, in_f, w, b, out_f, y, None)
    _each_null(call, ('x', 'w', 'y'))
    for name in ('rows', 'in_f', 'out_f'):
        assert call(**{name: 0}) == BADARG and call(**{name: -1}) == BADARG, name
    assert call(rows=2 ** 31 - 1, out_f=5) == UNSUPPORTED  # more than 2^31 - 1 workgroups


def test_fold_family_argument_checks(lib):
    def fold(fn):
        def call(src=PTR, b=2, nw=3, k=1, c=3, hw=5, dst=PTR):
            return fn(src, b, nw, k, c, hw, dst, None)
        return call
    for fn in (lib.sda_fold, lib.sda_fold_adjoint):
        call = fold(fn)
        _each_null(call, ('src', 'dst'))
        for name in ('b', 'nw', 'c', 'hw'):
            assert call(**{name: 0}) == BADARG and call(**{name: -1}) == BADARG, name
        assert call(k=-1) == BADARG

    def call(src=PTR, b=2, nw=3, k=1, c=3, hw=5, wct=9, dst=PTR):
        return lib.sda_unfold_adjoint(src, b, nw, k, c, hw, wct, dst, None)
    _each_null(call, ('src', 'dst'))
    for name in ('b', 'nw', 'c', 'hw'):
        assert call(**{name: 0}) == BADARG and call(**{name: -1}) == BADARG, name
    assert call(k=-1) == BADARG
    assert call(wct=8) == BADARG                           # a window row shorter than its (2k+1) c channels
    assert call(k=0, wct=2) == BADARG


def test_vp_schedule_argument_checks(lib):
    def call(t=PTR, ak=1, sk=0, out=PTR):
        return lib.sda_vp_schedule(t, ak, 1e-3, 1.5, sk, out, None)
    _each_null(call, ('t', 'out'))
    for kind in (-1, 3):
        assert call(ak=kind) == BADARG and call(sk=kind) == BADARG


def test_pc_and_guidance_argument_checks(lib):
    def predict(x=PTR, eps=PTR, numel=10):
        return lib.sda_pc_predict(x, eps, numel, 1.0, 0.5, None, None)
    _each_null(predict, ('x', 'eps'))
    assert predict(numel=0) == BADARG and predict(numel=-1) == BADARG

    def sumsq(eps=PTR, b=3, per=10, partial=PTR, nchunk=4):
        return lib.sda_sumsq_partial(eps, b, per, partial, nchunk, None)
    _each_null(sumsq, ('eps', 'partial'))
    for name in ('b', 'per', 'nchunk'):
        assert sumsq(**{name: 0}) == BADARG and sumsq(**{name: -1}) == BADARG, name
    assert sumsq(nchunk=1025) == BADARG
    assert sumsq(b=65536) == BADARG                        # the batch is grid.y

    def correct(x=PTR, eps=PTR, z=PTR, b=3, per=10, partial=PTR, nchunk=4):
        return lib.sda_pc_correct(x, eps, z, b, per, partial, nchunk, 0.5, 0.8, None, None)
    _each_null(correct, ('x', 'eps', 'z', 'partial'))
    for name in ('b', 'per', 'nchunk'):
        assert correct(**{name: 0}) == BADARG and correct(**{name: -1}) == BADARG, name
    assert correct(b=65536) == BADARG

    def denoise(x=PTR, eps=PTR, numel=10, xhat=PTR):
        return lib.sda_denoise(x, eps, numel, 0.8, 0.4, None, xhat, None)
    _each_null(denoise, ('x', 'eps', 'xhat'))
    assert denoise(numel=0) == BADARG and denoise(numel=-1) == BADARG

    def combine(eps=PTR, ghat=PTR, numel=10, out=PTR):
        return lib.sda_guided_combine(eps, ghat, PTR, numel, 0.8, 0.4, None, out, None)
    _each_null(combine, ('eps', 'ghat', 'out'))
    assert combine(numel=0) == BADARG and combine(numel=-1) == BADARG

    def cot(y=PTR, y_numel=5, ax=PTR, numel=10, out=PTR):
        return lib.sda_gauss_cotangent(y, y_numel, ax, numel, 0.3, 0.01, 0.8, 0.4, None, out, None)
    _each_null(cot, ('y', 'ax', 'out'))
    assert cot(numel=0) == BADARG and cot(y_numel=0) == BADARG and cot(numel=-5) == BADARG
    assert cot(y_numel=3) == BADARG and cot(y_numel=20) == BADARG            # y must tile ax exactly


def test_linear_argument_checks(lib):
    def call(x=PTR, rows=5, in_f=23, w=PTR, out_f=16, y=PTR):
        return lib.sda_linear(x, rows, in_f, w, None, out_f, 0, 0, 0, None, 0, None, y, None)
    _each_null(call, ('x', 'w', 'y'))
    for name in ('rows', 'in_f', 'out_f'):
        assert call(**{name: 0}) == BADARG and call(**{name: -1}) == BADARG, name


def test_row_ln_argument_checks(lib):
    def fwd(x=PTR, rows=5, f=64, unbiased=1, y=PTR):
        return lib.sda_row_ln(x, rows, f, 1e-5, unbiased, y, None, None, None)
    _each_null(fwd, ('x', 'y'))
    for name in ('rows', 'f'):
        assert fwd(**{name: 0}) == BADARG and fwd(**{name: -1}) == BADARG, name
    assert fwd(f=1025) == UNSUPPORTED and fwd(f=1025, unbiased=0) == UNSUPPORTED
    assert fwd(f=1, unbiased=1) == UNSUPPORTED             # an unbiased variance of one value divides by zero
    assert fwd(f=1025, y=None) == BADARG

    def bwd(gh=PTR, x=PTR, rows=5, f=64, mean=PTR, rstd=PTR, gx=PTR):
        return lib.sda_row_ln_bwd(gh, x, rows, f, mean, rstd, 1, None, gx, None)
    _each_null(bwd, ('gh', 'x', 'mean', 'rstd', 'gx'))
    for name in ('rows', 'f'):
        assert bwd(**{name: 0}) == BADARG and bwd(**{name: -1}) == BADARG, name
    assert bwd(f=1025) == UNSUPPORTED


def test_abi_version_is_unchanged(lib):
    assert lib.sda_abi_version() == 14
