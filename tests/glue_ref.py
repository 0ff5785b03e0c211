"""TEST-ONLY restatements of what csrc/elementwise.hip and csrc/linear.hip compute (numpy / torch float64 on the CPU; nothing from sda_amd
except in ``measure``, which is device only).

Two classes of kernel, two kinds of reference.

BIT-EXACT class -- the library is built with -ffp-contract=off and guide.hpp / sda_common.hpp state the order of operations, so the result is
determined: ``*_32`` functions evaluate the same operations in numpy float32 (every numpy float32 operation rounds once, as every device
operation does; division and square root are correctly rounded on both sides) and the GPU tests compare BITS.
    pc_predict_32, denoise_32, guided_combine_32, gauss_cotangent_32     the by-value and the coef_dev forms compute the same
    pc_correct_32                                                         given the partial sums the device produced
    fold_32, fold_adjoint_32                                              pure copies
    unfold_adjoint_32                                                     adds in j order, starting from 0.f
Their float64 twins (``*_64``, a ``V``) exist so that tests/test_glue_host.py can check each float32 restatement against a float64 bound
without a device.

BOUNDED class -- linear, linear_small, row_ln, row_ln_bwd, sumsq, time_embed, vp_schedule: the float64 value on the fp32 inputs with a
running first-order bound of the fp32 kernel's distance from it (``V`` of tests/step1d_ref.py: every correctly rounded operation adds
u |result|, u = 2^-24, to the propagated input errors), and
    a dot product / a sum   sum |w| err_in + (n + 2) u sum |w_i v_i| (+ |bias|): n terms in ANY order -- n - 1 additions, a product and a
                            bias each round once, so no chain is longer than n + 1; + 1 pays the second-order terms -- which covers the
                            MFMA tiles, the lane-strided partial sums and the shuffle trees without modelling them;
    cosf / sinf, expf, SiLU the allowances measured for tests/step1d_ref.py (TRIG_ULP, EXP_ULP, SILU_ULP; SiLU inside SILU_RANGE only);
    the other activations   no accuracy table of erff / expm1f / expf(-z^2 / 2) is recorded in the project, so each of sda_act's and
    and the derivatives     sda_dact's forms was MEASURED on an MI355X against the float64 function, through sda_linear with a 1 x 1
                            identity weight (act_in: y = act(x) 1 + 0;  dact_z: y = (1 . 1) act'(z)) so that nothing else contributes, over
                            SWEEP below (dense in [-ACT_RANGE, ACT_RANGE], plus 0, -0 and +-large), and doubled: ``MEASURED`` / ``ALLOW``.
                            Unit: u x mag(v) + TINY (1 + |v|), with mag the sum of the magnitudes of the function's terms (below; the value
                            itself where nothing cancels) and TINY = 2^-126, the smallest normal number: an intermediate below it may
                            lose all its bits (v_exp_f32 / v_rcp_f32 results, MFMA operands), and |v| is what it is multiplied by.

Every tolerance the two test modules use is one of these bounds or exact equality."""
import math

import numpy as np
import torch

from tests.step1d_ref import EXP_ULP, SILU_RANGE, SILU_ULP, TRIG_ULP, U, V, mu_sigma  # noqa: F401  (re-exported to the test modules)

F32 = np.float32
TINY = 2.0 ** -126
ACT_RANGE = 12.0
NONE, SILU, RELU, ELU, GELU, SELU = range(6)
ACT_NAMES = {NONE: 'none', SILU: 'SiLU', RELU: 'ReLU', ELU: 'ELU', GELU: 'GELU', SELU: 'SELU'}
SELU_L = 1.0507009873554804934193349852946
SELU_A = 1.6732632423543772848170429916717

#: worst error seen on the MI355X over ``sweep()``, in the unit above (``measure``); `d*` are the sda_dact forms.  ReLU and its derivative are
#: exact.  Worst arguments: elu -0.369, gelu 0.685, selu -0.411, dsilu -50 (the relative error of __expf grows with |z|; 9.9 inside
#: [-12, 12] would not cover it), delu -4.116, dgelu 1.022, dselu -1.889.
MEASURED = {'elu': 1.315, 'gelu': 2.175, 'selu': 2.623, 'dsilu': 19.776, 'delu': 1.304, 'dgelu': 1.997, 'dselu': 2.733}
#: 2 x MEASURED, rounded up: what the bounds use
ALLOW = {'elu': 2.63, 'gelu': 4.35, 'selu': 5.25, 'dsilu': 39.56, 'delu': 2.61, 'dgelu': 4.00, 'dselu': 5.47}
_ACT_KEY = {ELU: 'elu', GELU: 'gelu', SELU: 'selu'}
_DACT_KEY = {SILU: 'dsilu', ELU: 'delu', GELU: 'dgelu', SELU: 'dselu'}


def f64(a):
    """the fp32 operand as float64 (a torch tensor or anything numpy takes)"""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def f32(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _erf(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))).numpy()


def f64_tol(n, mag):
    """round-off of a float64 evaluation of n terms of magnitude mag: what two float64 restatements of one formula may differ by"""
    return (n + 2) * 2.0 ** -53 * 4 * np.asarray(mag, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ V helpers
def vdiv(a, b):
    a = a if isinstance(a, V) else V(a)
    b = b if isinstance(b, V) else V(b)
    assert (np.abs(b.v) > b.e).all(), 'a divisor whose bound reaches zero'
    v = a.v / b.v
    return V(v, (a.e + np.abs(v) * b.e) / (np.abs(b.v) - b.e) + U * np.abs(v))


def vsum(a: V, axis=-1, keepdims=False):
    """a sum of n terms in any order: n - 1 additions (+ 1: second order, and the zero a masked lane adds)"""
    n = a.v.shape[axis]
    mag = (np.abs(a.v) + a.e).sum(axis=axis, keepdims=keepdims)
    return V(a.v.sum(axis=axis, keepdims=keepdims), a.e.sum(axis=axis, keepdims=keepdims) + (n + 2) * U * mag)


def vdot(x: V, wop, bias=None):
    """x [rows][n] times wop [n][out] (float64, exact operands) plus bias, summed in any order"""
    aw = np.abs(wop)
    n = wop.shape[0]
    bias = np.zeros(wop.shape[1]) if bias is None else bias
    v = x.v @ wop + bias
    mag = (np.abs(x.v) + x.e) @ aw + np.abs(bias)
    return V(v, x.e @ aw + (n + 2) * U * mag)


# ------------------------------------------------------------------------------------------------ activations (sda_common.hpp)
def act_terms(a, v):
    """sda_act in float64 -> (value, derivative, magnitude of the terms)"""
    v = np.asarray(v, dtype=np.float64)
    if a == NONE:
        return v, np.ones_like(v), np.abs(v)
    if a == SILU:
        with np.errstate(over='ignore'):
            s = 1.0 / (1.0 + np.exp(-v))
        val = v * s
        return val, s * (1.0 + v * (1.0 - s)), np.abs(val)
    if a == RELU:
        return np.maximum(v, 0.0), (v > 0).astype(np.float64), np.abs(v)
    if a == ELU:
        neg = np.minimum(v, 0.0)
        val = np.where(v > 0, v, np.expm1(neg))
        return val, np.where(v > 0, 1.0, np.exp(neg)), np.abs(val)
    if a == GELU:
        er = _erf(v * math.sqrt(0.5))
        phi = np.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
        return 0.5 * v * (1.0 + er), 0.5 * (1.0 + er) + v * phi, 0.5 * np.abs(v) * (1.0 + np.abs(er))
    if a == SELU:
        neg = np.minimum(v, 0.0)
        val = SELU_L * np.where(v > 0, v, SELU_A * np.expm1(neg))
        return val, SELU_L * np.where(v > 0, 1.0, SELU_A * np.exp(neg)), np.abs(val)
    raise ValueError(a)


def dact_terms(a, z):
    """sda_dact in float64 -> (value, magnitude of the terms)"""
    z = np.asarray(z, dtype=np.float64)
    if a == SILU:
        with np.errstate(over='ignore'):
            s = 1.0 / (1.0 + np.exp(-z))
        return s * (1.0 + z * (1.0 - s)), s * (1.0 + np.abs(z) * (1.0 - s))
    if a == GELU:
        er = _erf(z * math.sqrt(0.5))
        phi = np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        return 0.5 * (1.0 + er) + z * phi, 0.5 * (1.0 + np.abs(er)) + np.abs(z) * phi
    if a in (NONE, RELU, ELU, SELU):
        d = act_terms(a, z)[1]
        return d, np.abs(d)
    raise ValueError(a)


def _in_range(a, v, e=0.0):
    top = float((np.abs(v) + e).max())
    if a == SILU and top > SILU_RANGE:
        raise ValueError(f'SiLU argument {top:.3g} beyond the range SILU_ULP was measured on')
    if a in (ELU, GELU, SELU) and top > ACT_RANGE:
        raise ValueError(f'activation argument {top:.3g} beyond the range its allowance was measured on')


def act_allowance(a, v, mag):
    """the device function's own error at an exact argument v"""
    if a in (NONE, RELU):
        return np.zeros_like(mag)
    ulp = SILU_ULP if a == SILU else ALLOW[_ACT_KEY[a]]
    return ulp * U * mag + TINY * (1.0 + np.abs(v))


def act_v(a, x: V) -> V:
    """sda_act of a bounded value: the steepest slope over [v - e, v + e] (the derivative at both ends and in the middle, + 2 e for its
    change in between: |act''| <= 2 for all five; ReLU's and SELU's jumps at 0 are inside whenever the interval straddles 0) times e,
    plus the function's own allowance"""
    if a == NONE:
        return x
    _in_range(a, x.v, x.e)
    val, d, mag = act_terms(a, x.v)
    slope = np.maximum(np.abs(d), np.maximum(np.abs(act_terms(a, x.v - x.e)[1]), np.abs(act_terms(a, x.v + x.e)[1]))) + 2.0 * x.e
    return V(val, slope * x.e + act_allowance(a, x.v, mag))


def dact_v(a, z) -> V:
    """sda_dact at an exact fp32 argument"""
    z = np.asarray(z, dtype=np.float64)
    val, mag = dact_terms(a, z)
    if a in (NONE, RELU):
        return V(val)
    if float(np.abs(z).max()) > ACT_RANGE:
        raise ValueError('derivative argument beyond the range its allowance was measured on')
    return V(val, ALLOW[_DACT_KEY[a]] * U * mag + TINY * (1.0 + np.abs(z)))


# ------------------------------------------------------------------------------------------------ linear.hip
def linear_64(x, w, b=None, trans_w=False, act_in=NONE, act_out=NONE, dact_z=None, act_d=NONE, res=None) -> V:
    """sda_linear: (act_out)(act_in(x) Wop + b) * act_d'(z) + res;  w is [out][in], or [in][out] with trans_w"""
    a = act_v(act_in, V(f64(x)))
    wop = f64(w) if trans_w else f64(w).T
    y = vdot(a, wop, None if b is None else f64(b))
    y = act_v(act_out, y)
    if dact_z is not None:
        y = y * dact_v(act_d, f64(dact_z))
    if res is not None:
        y = y + V(f64(res))
    return y


def linear_small_64(x, w, b=None) -> V:
    return vdot(V(f64(x)), f64(w).T, None if b is None else f64(b))


def row_ln_64(x, eps, unbiased):
    """sda_row_ln -> (y [rows][f], mean [rows], rstd [rows]) as V.  The mean's error enters every x - mean, so a row whose mean dwarfs its
    spread gets the bound its conditioning deserves: (f + 2) u sum |x| / f on a difference of size sigma."""
    x = V(f64(x))
    f = x.v.shape[1]
    m = vdiv(vsum(x, axis=1, keepdims=True), float(f))
    dlt = x - m
    q = vsum(dlt * dlt, axis=1, keepdims=True)
    var = vdiv(q, float(f - 1 if unbiased else f))
    r = vdiv(1.0, (var + float(F32(eps))).sqrt())
    y = dlt * r
    return y, V(m.v[:, 0], m.e[:, 0]), V(r.v[:, 0], r.e[:, 0])


def row_ln_bwd_64(gh, x, mean, rstd, unbiased, res=None, exact_stats=False) -> V:
    """sda_row_ln_bwd on the mean and rstd it is GIVEN (fp32: exact operands; exact_stats: float64 ones, for the host test)"""
    g, x = V(f64(gh)), V(f64(x))
    f = x.v.shape[1]
    m, r = (V(np.asarray(a, dtype=np.float64)[:, None]) if exact_stats else V(f64(a)[:, None]) for a in (mean, rstd))
    h = (x - m) * r
    s1 = vdiv(vsum(g, axis=1, keepdims=True), float(f))
    s2 = vdiv(vsum(g * h, axis=1, keepdims=True), float(f - 1 if unbiased else f))
    v = r * ((g - s1) - h * s2)
    if res is not None:
        v = v + V(f64(res))
    return v


# ------------------------------------------------------------------------------------------------ elementwise.hip, bounded class
def sumsq_64(eps) -> V:
    """sum of squares over the last axis, in any order and any chunking"""
    e = V(f64(eps))
    return vsum(e * e, axis=-1)


def silu_v(x: V) -> V:
    return act_v(SILU, x)


def time_embed_64(t, freqs, w0, b0, w2, b2) -> V:
    """sda_time_embed: [cos(f t), sin(f t)] -> Linear -> SiLU -> Linear, emb [nt][e]"""
    t, freqs = f64(t).reshape(-1), f64(freqs)
    ang = V(freqs[None, :]) * V(t[:, None])
    c, s = ang.cos(), ang.sin()
    feat = V(np.concatenate([c.v, s.v], axis=1), np.concatenate([c.e, s.e], axis=1))
    hid = silu_v(vdot(feat, f64(w0).T, f64(b0)))
    return vdot(hid, f64(w2).T, f64(b2))


def vp_64(t, alpha_kind, eta, k, sigma_kind):
    """mu(t), sigma(t) in plain float64 on the arguments as given (no rounding of eta or k): the formula ``mu_sigma`` bounds"""
    t = np.asarray(t, dtype=np.float64)
    a = (1.0 - (1.0 - eta) * t, np.cos(k * t) ** 2, np.exp(k * t * t))[alpha_kind]
    sg = (np.sqrt(1.0 - a * a + eta * eta), 1.0 - a * a + eta, 1.0 - a + eta)[sigma_kind]
    return a, sg


# ------------------------------------------------------------------------------------------------ elementwise.hip, bit-exact class
def guide_32(mu, sigma, std=0.0, gamma=0.0):
    """sda_guide's per-launch constants (guide.hpp) -> (mu, sigma, kk, var), all float32"""
    mu, sg, std, gamma = F32(mu), F32(sigma), F32(std), F32(gamma)
    with np.errstate(divide='ignore', invalid='ignore'):
        kk = sg / mu
        rr = sg / mu
    var = std * std + gamma * (rr * rr)
    return mu, sg, kk, F32(var)


def pc_predict_32(x, eps, r, c1):
    return F32(r) * f32(x) + F32(c1) * f32(eps)


def denoise_32(x, eps, mu, sigma):
    mu, sg, _, _ = guide_32(mu, sigma)
    return (f32(x) - sg * f32(eps)) / mu


def guided_combine_32(eps, ghat, vjp, mu, sigma):
    _, sg, kk, _ = guide_32(mu, sigma)
    inner = f32(ghat) - (F32(0.0) if vjp is None else sg * f32(vjp))
    return f32(eps) - kk * inner


def gauss_cotangent_32(y, ax, std, gamma, mu, sigma):
    """y broadcasts over ax's leading axis (flat index i % y_numel)"""
    _, _, _, var = guide_32(mu, sigma, std, gamma)
    ax = f32(ax)
    yb = np.resize(f32(y).reshape(-1), ax.size).reshape(ax.shape)
    return (yb - ax) / var


def pc_correct_32(x, eps, z, partial, tau, sigma):
    """x, eps, z [b][per], partial [b][nchunk] as the device wrote it: the chunk sums are added in index order from 0.f"""
    x, eps, z, partial = f32(x), f32(eps), f32(z), f32(partial)
    per = x.shape[1]
    tot = np.zeros(x.shape[0], dtype=np.float32)
    for j in range(partial.shape[1]):
        tot = tot + partial[:, j]
    delta = F32(tau) / (tot / F32(per))
    sq = np.sqrt(F32(2.0) * delta)
    out = x - (delta[:, None] * eps + sq[:, None] * z) * F32(sigma)
    assert out.dtype == np.float32
    return out


def fold_32(s, k, c):
    """s [b][nw][(2k+1) c (+ nothing)][hw] -> [b][nw + 2k][c][hw]: the first window's leading slots, every centre, the last window's tail"""
    b, nw = s.shape[:2]
    s5 = s.reshape(b, nw, 2 * k + 1, c, -1)
    return np.concatenate([s5[:, 0, :k], s5[:, :, k], s5[:, nw - 1, k + 1:]], axis=1)


def fold_adjoint_32(g, nw, k):
    """g [b][nw + 2k][c][hw] -> [b][nw][2k+1][c][hw]: the cotangent where fold read, 0.f elsewhere"""
    b, L, c, hw = g.shape
    gs = np.zeros((b, nw, 2 * k + 1, c, hw), dtype=g.dtype)
    gs[:, :, k] = g[:, k:k + nw]
    gs[:, 0, :k] = g[:, :k]
    gs[:, nw - 1, k + 1:] = g[:, nw + k:]
    return gs


def unfold_adjoint_32(gwin, k, c):
    """gwin [b][nw][win_c_total][hw] (channels past (2k+1) c are never read) -> [b][nw + 2k][c][hw], slot j added in ascending order"""
    b, nw, _, hw = gwin.shape
    gx = np.zeros((b, nw + 2 * k, c, hw), dtype=gwin.dtype)
    for j in range(2 * k + 1):
        gx[:, j:j + nw] = gx[:, j:j + nw] + gwin[:, :, j * c:(j + 1) * c]
    return gx


# ---- the float64 twins of the bit-exact class (host test only)
def pc_predict_64(x, eps, r, c1) -> V:
    return V(float(F32(r))) * V(f64(x)) + V(float(F32(c1))) * V(f64(eps))


def denoise_64(x, eps, mu, sigma) -> V:
    return vdiv(V(f64(x)) - V(float(F32(sigma))) * V(f64(eps)), float(F32(mu)))


def guided_combine_64(eps, ghat, vjp, mu, sigma) -> V:
    sg = V(float(F32(sigma)))
    kk = vdiv(sg, float(F32(mu)))
    inner = V(f64(ghat)) if vjp is None else V(f64(ghat)) - sg * V(f64(vjp))
    return V(f64(eps)) - kk * inner


def gauss_cotangent_64(y, ax, std, gamma, mu, sigma) -> V:
    rr = vdiv(V(float(F32(sigma))), float(F32(mu)))
    var = V(float(F32(std))) * V(float(F32(std))) + V(float(F32(gamma))) * (rr * rr)
    ax = f64(ax)
    yb = np.resize(f64(y).reshape(-1), ax.size).reshape(ax.shape)
    return vdiv(V(yb) - V(ax), var)


def pc_correct_64(x, eps, z, partial, tau, sigma) -> V:
    x, eps, z = V(f64(x)), V(f64(eps)), V(f64(z))
    per = x.v.shape[1]
    tot = vsum(V(f64(partial)), axis=1, keepdims=True)
    delta = vdiv(float(F32(tau)), vdiv(tot, float(per)))
    sq = (V(2.0) * delta).sqrt()
    return x - (delta * eps + sq * z) * V(float(F32(sigma)))


def unfold_adjoint_64(gwin, k, c) -> V:
    g = f64(gwin)
    b, nw, _, hw = g.shape
    terms = np.zeros((2 * k + 1, b, nw + 2 * k, c, hw))
    for j in range(2 * k + 1):
        terms[j, :, j:j + nw] = g[:, :, j * c:(j + 1) * c]
    return vsum(V(terms), axis=0)


# ------------------------------------------------------------------------------------------------ measuring the allowances (device only)
def sweep():
    """fp32 arguments: 2^16 + 1 evenly spaced over [-ACT_RANGE, ACT_RANGE] (0 among them), -0, the neighbours of 0, and +-large"""
    dense = np.linspace(-ACT_RANGE, ACT_RANGE, 2 ** 16 + 1, dtype=np.float64).astype(np.float32)
    special = [0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 1e-3, -1e-3, 20.0, -20.0, 50.0, -50.0, 87.0, -87.0, 89.0, -89.0, 100.0, -100.0,
               104.0, -104.0, 1e4, -1e4, 1e30, -1e30]
    return np.concatenate([dense, np.asarray(special, dtype=np.float32)])


def measure(dev='cuda:0'):
    """Device only: the worst error of sda_act's ELU / GELU / SELU and sda_dact's SiLU' / ELU' / GELU' / SELU' over ``sweep()`` in the
    module's unit (u mag + TINY (1 + |v|)), seen through sda_linear with a 1 x 1 identity weight -> what MEASURED holds, and the argument
    of each worst case.  (ReLU, its derivative and act 0 are asserted exact.)"""
    from sda_amd import ops
    v32 = sweep()
    v = v32.astype(np.float64)
    xd = torch.from_numpy(v32).to(dev).reshape(-1, 1)
    one = torch.ones(1, 1, device=dev)
    ones = torch.ones_like(xd)
    worst, where = {}, {}

    def note(key, got, val, mag):
        got = got.double().cpu().numpy().reshape(-1)
        assert np.isfinite(got).all(), key
        ratio = np.abs(got - val) / (U * mag + TINY * (1.0 + np.abs(v)))
        i = int(ratio.argmax())
        worst[key], where[key] = float(ratio[i]), float(v32[i])

    for a, key in _ACT_KEY.items():
        val, _, mag = act_terms(a, v)
        note(key, ops.linear(xd, one, None, act_in=a), val, mag)
    for a, key in _DACT_KEY.items():
        val, mag = dact_terms(a, v)
        note(key, ops.linear(ones, one, None, dact_z=xd, act_d=a), val, mag)
    for a in (NONE, RELU):
        got = ops.linear(xd, one, None, act_in=a).double().cpu().numpy().reshape(-1)
        assert np.array_equal(got, act_terms(a, v)[0]), a
        got = ops.linear(ones, one, None, dact_z=xd, act_d=a).double().cpu().numpy().reshape(-1)
        assert np.array_equal(got, dact_terms(a, v)[0]), a
    return worst, where
