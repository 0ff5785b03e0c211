"""TEST-ONLY numpy restatement of sda_amd/csrc/chain.hip: the RK4 transitions of the three built-in systems in the reference's
operation order (fp32 or float64 by the dtype of the input), the noisy transition (noise = philox_ref.randn_rows), the
affine-select log-weights, the float64 CDF with its ancestor search (uniforms = philox_ref), and the reference filter's history
handling LITERALLY -- concatenate, then x = x[j] (sda/utils.py:193-200)."""
import numpy as np

from tests import philox_ref

KINDS = {'Lorenz63': 'lorenz63', 'NoisyLorenz63': 'lorenz63', 'Lorenz96': 'lorenz96', 'LotkaVolterra': 'lotka_volterra'}


def f(kind, p, x):
    t = x.dtype.type
    if kind == 'lorenz63':
        s, r, b = (t(v) for v in p)
        return np.stack((s * (x[..., 1] - x[..., 0]), x[..., 0] * (r - x[..., 2]) - x[..., 1], x[..., 0] * x[..., 1] - b * x[..., 2]), -1)
    if kind == 'lotka_volterra':
        a, b, d, g = (t(v) for v in p)
        return np.stack((a - b * np.exp(x[..., 1]), d * np.exp(x[..., 0]) - g), -1)
    if kind == 'lorenz96':
        x1, x2, x3 = (np.roll(x, i, axis=-1) for i in (1, -2, -1))
        return (x1 - x2) * x3 - x + t(p[0])
    raise ValueError(kind)


def transition(kind, p, dt, steps, x):
    """One DiscreteODE.transition: `steps` RK4 sub-steps of dt / steps (the python scalar is rounded to x's dtype once)."""
    t = x.dtype.type
    h, two, six = t(dt / steps), t(2), t(6)
    for _ in range(steps):
        k1 = f(kind, p, x)
        k2 = f(kind, p, x + h * k1 / two)
        k3 = f(kind, p, x + h * k2 / two)
        k4 = f(kind, p, x + h * k3)
        x = x + h * (k1 + two * k2 + two * k3 + k4) / six
    return x


def trajectory(kind, p, dt, steps, x, length, noise_std=0.0, seed=0, row0=0, draw0=0):
    """(length, m, d): the states after each transition; noise_std > 0 adds noise_std * randn_rows(m, d, seed, row0, draw0 + t)."""
    out = []
    for t in range(length):
        x = transition(kind, p, dt, steps, x)
        if noise_std > 0:
            x = x + x.dtype.type(noise_std) * philox_ref.randn_rows(x.shape[0], x.shape[1], seed, row0, draw0 + t).astype(x.dtype)
        out.append(x)
    return np.stack(out)


def normal_log_prob(v, mu, s):
    v, mu = np.asarray(v, np.float64), np.asarray(mu, np.float64)
    return -((v - mu) ** 2) / (2 * s * s) - np.log(s) - 0.5 * np.log(2 * np.pi)


def logweights(x, index, shift, scale, sigma, y):
    """float64 log-weights of states x (m, d) for A(x) = (x[index] - shift) / scale observed as y (k,)."""
    a = (np.asarray(x, np.float64)[:, index] - np.asarray(shift, np.float64)) / np.asarray(scale, np.float64)
    return normal_log_prob(a, np.asarray(y, np.float64), float(sigma)).sum(-1)


def uniforms(m, seed, obs):
    """u_j in (0, 1) of observation `obs`: counter {j, obs, 0x80000000 | j_hi, 'RESA'}, 52 bits and a set 53rd."""
    w0, w1, _, _ = philox_ref.philox4x32_10(np.arange(m, dtype=np.uint64), obs, 0x80000000, 0x52455341, seed & 0xffffffff,
                                            (seed >> 32) & 0xffffffff)
    v = ((w0.astype(np.uint64) >> np.uint64(6)) << np.uint64(26)) | (w1.astype(np.uint64) >> np.uint64(6))
    return (2 * v + 1).astype(np.float64) * 2.0 ** -53


def ancestors(w, seed, obs, return_margin=False):
    """The ancestors of fp32 weights w: float64 cumulative sum, smallest i with cdf[i] > u cdf[-1] (searchsorted, side=right)."""
    cdf = np.cumsum(np.asarray(w, np.float64))
    target = uniforms(len(cdf), seed, obs) * cdf[-1]
    anc = np.minimum(np.searchsorted(cdf, target, side='right'), len(cdf) - 1).astype(np.int32)
    if return_margin:
        # distance of every target to the nearest cdf value, in units of the total: a draw this close to a boundary may land
        # on either side when the prefix sums are formed in another order
        i = np.searchsorted(cdf, target, side='right')
        near = np.stack((cdf[np.minimum(i, len(cdf) - 1)], cdf[np.maximum(i - 1, 0)]))
        margin = np.abs(near - target).min(axis=0) / cdf[-1]
        return anc, cdf, target, margin
    return anc


def regather(S, anc, step):
    """The reference's history handling, literally: x grows by concatenation, and after every observation x = x[j].
    S (T + 1, m, d) holds the states as the filter produced them (slot s of segment k continues slot anc[k - 1][s] of the
    re-gathered history), anc (N, m).  Returns (m, T + 1, d)."""
    x = S[0][:, None]
    for k in range(anc.shape[0]):
        for t in range(k * step + 1, (k + 1) * step + 1):
            x = np.concatenate((x, S[t][:, None]), axis=1)
        x = x[anc[k]]
    return x
