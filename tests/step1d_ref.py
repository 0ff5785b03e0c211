"""TEST-ONLY float64 restatements of what csrc/step1d.hip computes, with a running fp32 error bound for the step prologue.

Prologue (``prologue``): from the fp32 inputs, mu / sigma of the 3 x 3 stock schedules (sda/score.py:195-210, 279-302), the features
[cos(f t), sin(f t)], Linear -> SiLU -> Linear and the projection, all in float64.  Beside every value runs a first-order bound of the
fp32 kernel's distance from it, with u = 2^-24 the unit round-off of one correctly rounded fp32 operation (+, -, *, /, sqrt):

    scalar operations   every fp32 operation adds u |result| to the propagated input errors;
    features            |sin or cos of the angle| x |f t| u  (the angle f t is rounded once)  +  TRIG_ULP u |value|;
    a dot product       sum |w| err_in + (chain + 2) u (sum |w v| + |bias|): `chain` is the longest chain of additions of the kernel's
                        summation order -- ceil(n / 8) + 3 for sda_dot8 (n / 8 per partial sum, a three-level tree), ceil(n / 64) + 6 for
                        the wave-per-output projection (strided partial sums, a six-level tree) -- and + 2 are the product and the bias;
    SiLU                |silu'(v)| err_v + SILU_ULP u |silu(v)|  (device: v x v_rcp_f32(1 + __expf(-v))), for |v| <= SILU_RANGE only
                        (the error of __expf grows with |v|; ``prologue`` raises beyond);
    cos / exp schedule  |f'(arg)| err_arg + TRIG_ULP (EXP_ULP) u |value|.

The three *_ULP allowances are the only constants that are not derived here: per call, in units of u |true value|.  No accuracy table of
the device library's cosf / sinf / expf is at hand, so they were MEASURED on an MI355X through the three unfused kernels (never through
the prologue), at the arguments the tests use, and doubled:

    function            measured through                                                      worst observed      used
    cosf, sinf          sda_time_embed with w0 = +-2^30 selectors: SiLU is the identity       1.608               3.22
                        beyond v = 17, so the embedding IS the feature (all pi j t of the
                        tests, j <= 2, 4, 13, 16, 64, and cos(k t) of the schedule tests)
    expf                sda_vp_schedule, alpha 'exp' (mu = expf(k t^2)), 263 t in [0, 1]      1.097               2.20
    SiLU                sda_time_embed at t = 0 (cos = 1 exactly): emb = silu(w0[:, 0]),      8.512               17.03
                        8192 values in [-8, 8)

``mc_finish``: the tail of the fused local route from guide.hpp's formulas in float64 -- gx[l] = sum_j gwin[l - j][j c + ch], vjp = bare ?
gx : ghat cx + gx with cx = cx0 + cx1 sigma, out = eps - (sigma / mu)(ghat - sigma vjp), mode 1: x <- r x + c1 out, mode 2: partial[b] =
sum out^2 -- with the magnitude |eps| + kk |ghat| + kk sigma (|ghat cx| + sum |gwin terms|) its tolerance is stated in."""
import numpy as np

U = 2.0 ** -24

#: worst observed error on the MI355X, in u |true value| per call: what `measure` below returned at the arguments of tests/test_gpu_step1d.py
MEASURED = {'trig': 1.608, 'exp': 1.097, 'silu': 8.512}
TRIG_ULP = 3.22             # 2 x MEASURED, rounded up
EXP_ULP = 2.20
SILU_ULP = 17.03
SILU_RANGE = 8.0


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


class V:
    """A float64 value (array) with a bound of the fp32 computation's distance from it."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    def _r(self, v, e):                     # one correctly rounded operation
        return V(v, e + U * np.abs(v))

    def __add__(self, o):
        o = o if isinstance(o, V) else V(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = o if isinstance(o, V) else V(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V(o) - self

    def __mul__(self, o):
        o = o if isinstance(o, V) else V(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def sqrt(self):
        v = np.sqrt(self.v)
        lo = np.sqrt(np.maximum(self.v - self.e, 0.0))           # (exact propagation: sqrt is steep near 0)
        hi = np.sqrt(self.v + self.e)
        return self._r(v, np.maximum(v - lo, hi - v))

    def cos(self):
        v = np.cos(self.v)
        return V(v, np.minimum(np.abs(np.sin(self.v)) * self.e + 0.5 * self.e ** 2, 2.0) + TRIG_ULP * U * np.abs(v))

    def sin(self):
        v = np.sin(self.v)
        return V(v, np.minimum(np.abs(np.cos(self.v)) * self.e + 0.5 * self.e ** 2, 2.0) + TRIG_ULP * U * np.abs(v))

    def exp(self):
        v = np.exp(self.v)
        return V(v, v * np.expm1(self.e) + EXP_ULP * U * v)


def mu_sigma(t, alpha_kind, eta, k, sigma_kind):
    """sda_vp_mu_sigma (csrc/sda_common.hpp) in float64 on the fp32 t, eta, k: (mu, sigma) as V."""
    t, eta, k = V(_f64(t)), float(np.float32(eta)), float(np.float32(k))
    if alpha_kind == 0:
        a = 1.0 - (1.0 - V(eta)) * t
    elif alpha_kind == 1:
        c = (V(k) * t).cos()
        a = c * c
    else:
        a = (V(k) * (t * t)).exp()
    if sigma_kind == 0:
        sg = ((1.0 - a * a) + V(eta) * V(eta)).sqrt()
    elif sigma_kind == 1:
        sg = (1.0 - a * a) + V(eta)
    else:
        sg = (1.0 - a) + V(eta)
    return a, sg


def _dot(w, x: V, bias, chain):
    """rows of w (float64 [out][in]) times x ([nt][in]) plus bias, summed in some order whose longest chain of additions is `chain`."""
    aw = np.abs(w)
    v = x.v @ w.T + bias
    mag = np.abs(x.v) @ aw.T + np.abs(bias)
    return V(v, x.e @ aw.T + (chain + 2) * U * mag)


def silu(x: V):
    if np.abs(x.v).max() + x.e.max() > SILU_RANGE:
        raise ValueError(f'pre-activation {np.abs(x.v).max():.3g} beyond the range SILU_ULP was measured on')
    s = 1.0 / (1.0 + np.exp(-x.v))
    v = x.v * s
    d = np.abs(s * (1.0 + x.v * (1.0 - s)))
    return V(v, (d + 0.25 * x.e) * x.e + SILU_ULP * U * np.abs(v))        # (|silu''| <= 1/2: the second-order term)


def prologue(t, sched, freqs, w0, b0, w2, b2, wp=None, bp=None):
    """-> dict(mu, sigma: V [nt];  emb: V [nt][e];  mod: V [nt][cp], or emb without a projection)."""
    ak, eta, k, sk = sched
    t = _f64(t).reshape(-1)
    freqs, w0, b0, w2, b2 = (_f64(a) for a in (freqs, w0, b0, w2, b2))
    mu, sg = mu_sigma(t, ak, eta, k, sk)
    ang = V(freqs[None, :]) * V(t[:, None])
    c, s = ang.cos(), ang.sin()
    feat = V(np.concatenate([c.v, s.v], axis=1), np.concatenate([c.e, s.e], axis=1))
    nin, hidden, e = w0.shape[1], w0.shape[0], w2.shape[0]
    hid = silu(_dot(w0, feat, b0, -(-nin // 8) + 3))
    emb = _dot(w2, hid, b2, -(-hidden // 8) + 3)
    mod = emb
    if wp is not None:
        mod = _dot(_f64(wp), emb, _f64(bp), -(-e // 64) + 6)
    return dict(mu=mu, sigma=sg, emb=emb, mod=mod)


def measure(times, nfs, k_cos, k_exp, eta=1e-3, dev='cuda:0'):
    """Device only: the worst error of cosf / sinf, expf and SiLU in u |true value|, seen through the UNFUSED kernels (docstring above) at
    the angles pi j t (j <= nf) and k_cos t, the exponents k_exp t^2 and 8192 SiLU arguments in [-SILU_RANGE, SILU_RANGE] -> MEASURED's dict."""
    import torch
    from sda_amd import ops
    t32 = np.asarray(times, dtype=np.float32)
    td = torch.tensor(t32, device=dev)
    worst = {'trig': 0.0, 'exp': 0.0, 'silu': 0.0}
    scale = 2.0 ** 30
    for fr in [(np.pi * np.arange(1, nf + 1)).astype(np.float32) for nf in nfs] + [np.asarray([k_cos], dtype=np.float32)]:
        n = len(fr)
        w0 = np.zeros((4 * n, 2 * n), dtype=np.float32)                 # rows 2f, 2f + 1: +-2^30 on feature f
        for f in range(2 * n):
            w0[2 * f, f], w0[2 * f + 1, f] = scale, -scale
        eye = torch.eye(4 * n, device=dev)
        zero = torch.zeros(4 * n, device=dev)
        emb = ops.time_embed(td, torch.tensor(fr, device=dev), torch.tensor(w0, device=dev), zero, eye, zero).cpu().numpy().astype(np.float64)
        feat = (emb[:, 0::2] - emb[:, 1::2]) / scale                    # (one of the pair is the feature x 2^30, the other -0)
        ang = (fr[None, :] * t32[:, None]).astype(np.float64)           # fp32 product, as the kernel forms it
        ref = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
        ok = np.abs(ref) * scale > 32.0
        worst['trig'] = max(worst['trig'], float((np.abs(feat - ref)[ok] / (U * np.abs(ref[ok]))).max()))
    tt = np.unique(np.concatenate([t32, np.linspace(0.0, 1.0, 257, dtype=np.float32)]))
    k32 = np.float32(k_exp)
    for tv in tt:
        mu = ops.vp_schedule(torch.tensor([tv], device=dev), 2, eta, float(k32), 2)[0].item()
        ref = np.exp(np.float64(k32 * np.float32(tv * tv)))
        worst['exp'] = max(worst['exp'], abs(mu - ref) / (U * ref))
    v = np.linspace(-SILU_RANGE, SILU_RANGE, 8193, dtype=np.float32)[:8192].reshape(8, 1024)
    eye, zero = torch.eye(1024, device=dev), torch.zeros(1024, device=dev)
    for row in v:
        w0 = np.stack([row, np.zeros_like(row)], axis=1)                # feat(t = 0) = [cos 0, sin 0] = [1, 0]
        emb = ops.time_embed(torch.zeros(1, device=dev), torch.tensor([np.pi], dtype=torch.float32, device=dev), torch.tensor(w0, device=dev),
                             zero, eye, zero).cpu().numpy().astype(np.float64)[0]
        x = row.astype(np.float64)
        ref = x / (1.0 + np.exp(-x))
        ok = ref != 0.0
        worst['silu'] = max(worst['silu'], float((np.abs(emb - ref)[ok] / (U * np.abs(ref[ok]))).max()))
    return worst


def mc_finish(eps, ghat, gwin, nw, k, c, cx0, cx1, mu, sigma, mode=0, xs=None, step_coef=None):
    """eps, ghat [b][L][c], gwin [b nw][gld], all fp32 -> dict(out, mag [b][L][c] float64; x (mode 1); partial [b] (mode 2))."""
    eps, ghat, gwin = _f64(eps), _f64(ghat), _f64(gwin)
    b, L = eps.shape[0], nw + 2 * k
    mu, sigma, cx0, cx1 = (float(np.float32(v)) for v in (mu, sigma, cx0, cx1))
    g = gwin.reshape(b, nw, -1)
    gx = np.zeros((b, L, c))
    gmag = np.zeros((b, L, c))
    for j in range(2 * k + 1):
        gx[:, j:j + nw] += g[:, :, j * c:(j + 1) * c]
        gmag[:, j:j + nw] += np.abs(g[:, :, j * c:(j + 1) * c])
    bare = cx0 == 0.0 and cx1 == 0.0
    cx = cx0 + cx1 * sigma
    vjp = gx if bare else ghat * cx + gx
    kk = sigma / mu
    out = eps - kk * (ghat - sigma * vjp)
    res = dict(out=out, mag=np.abs(eps) + abs(kk) * np.abs(ghat) + abs(kk * sigma) * ((0.0 if bare else np.abs(ghat * cx)) + gmag))
    if mode == 1:
        r, c1 = (float(v) for v in _f64(step_coef)[:2])
        res['x'] = r * _f64(xs) + c1 * out
    if mode == 2:
        res['partial'] = (out ** 2).reshape(b, -1).sum(axis=1)
    return res
