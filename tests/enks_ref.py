"""TEST-ONLY numpy replay of one analysis of the stochastic ensemble Kalman smoother (the five steps of include/sda_hip.h,
csrc/enks.hip) in a chosen dtype, the cases the CPU and GPU tests share, and a float64 replay of the whole smoother on the damped
spring.  ``analysis(.., np.float64)`` is the reference; the same call in float32 gives the 'own error' of the project's bound rule
(tests/chain_util.bound)."""
import ctypes
import functools

import numpy as np

from tests import philox_ref

SALT = 0x454E4B53

#: (M, d, k) -> what the case exercises
SHAPES = [(2, 3, 1), (67, 3, 1), (1000, 5, 3), (256, 40, 20), (130, 64, 64)]
#: (slabs of S, lo, t): a window of 1 slab, of 2 slabs, and of 9 slabs where lag = 4 at step 2 clips slabs 0 and 1 away
WINDOWS = [(3, 1, 1), (4, 1, 2), (12, 2, 10)]
INFLATIONS = [1.0, 1.05]
SIGMAS = [1e-3, 1.0]


def observation(m, d, k):
    """(index, shift, scale) of the case: trivial at the minimum ensemble, a non-trivial shift / scale, a repeated and unordered
    index, every other component, and a reversed full selection with varying shift and scale."""
    if (m, d, k) == (2, 3, 1):
        return [0], [0.0], [1.0]
    if (m, d, k) == (67, 3, 1) or (d, k) == (3, 1):
        return [2], [25.0], [8.6]
    if (d, k) == (5, 3):
        return [4, 1, 4], [0.5, -1.0, 0.25], [2.0, 0.5, 3.0]
    if (d, k) == (40, 20):
        return list(range(0, 40, 2)), [0.0] * 20, [1.0] * 20
    if (d, k) == (64, 64):
        return list(range(63, -1, -1)), [0.1 * (i % 7) for i in range(64)], [1.0 + 0.25 * (i % 5) for i in range(64)]
    raise KeyError((m, d, k))


def perturbations(m, k, seed, draw):
    """(m, k) float32: eps of member j at observation `draw`, the salted sda_randn_rows stream."""
    return philox_ref.randn_rows(m, k, seed ^ SALT, 0, draw)


def obs_apply(x, index, shift, scale, dtype):
    return (x[..., index] - np.asarray(shift, np.float32).astype(dtype)) / np.asarray(scale, np.float32).astype(dtype)


def analysis(S, lo, t, index, shift, scale, sigma, y, eps, inflation, dtype):
    """One analysis on a copy of S (slabs, M, d): returns (S', a (k, M), z (k, M)) in `dtype`.  Every parameter is first rounded to
    float32, as the device receives it."""
    S = np.array(S, dtype=dtype)
    m = S.shape[1]
    sigma = dtype(np.float32(sigma))
    lam = dtype(np.float32(inflation))
    y = np.asarray(y, np.float32).astype(dtype)
    eps = np.asarray(eps, np.float32).astype(dtype)
    if np.float32(inflation) != np.float32(1.0):                      # step 1
        mean = S[t].mean(axis=0, dtype=dtype)
        S[t] = mean + lam * (S[t] - mean)
    h = obs_apply(S[t], index, shift, scale, dtype)                   # step 2
    a = h - h.mean(axis=0, dtype=dtype)
    k = a.shape[1]
    C = a.T @ a / dtype(m - 1) + sigma * sigma * np.eye(k, dtype=dtype)      # step 3
    z = np.linalg.solve(C, ((y + sigma * eps) - h).T).T.astype(dtype)        # step 4
    for s in range(lo, t + 1):                                        # step 5
        xs = S[s]
        P = (xs - xs.mean(axis=0, dtype=dtype)).T @ a / dtype(m - 1)
        S[s] = xs + z @ P.T
    return S, np.ascontiguousarray(a.T), np.ascontiguousarray(z.T)


@functools.lru_cache(None)
def case(m, d, k, slabs, lo, t, inflation, sigma, seed=1234):
    """Inputs and both replays of one case, computed once and shared: dict(S, y, eps, obs, ref64, ref32)."""
    rng = np.random.default_rng([seed, m, d, k, slabs])
    base = rng.standard_normal((m, d))
    S = (base[None] * np.linspace(0.5, 1.5, slabs)[:, None, None] + 0.5 * rng.standard_normal((slabs, m, d)) + 1.0).astype(np.float32)
    index, shift, scale = observation(m, d, k)
    y = (obs_apply(S[t].astype(np.float64).mean(axis=0), index, shift, scale, np.float64) + 0.3 * rng.standard_normal(k)).astype(np.float32)
    draw = 3
    eps = perturbations(m, k, seed, draw)
    args = (S, lo, t, index, shift, scale, sigma, y, eps, inflation)
    out = dict(S=S, y=y, eps=eps, obs=(index, shift, scale), seed=seed, draw=draw, ref64=analysis(*args, np.float64),
               ref32=analysis(*args, np.float32))
    for v in (S, y, eps):
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------- the damped spring, float64
def spring_matrices():
    """(A, b, Lq, m0, L0) float64 of chains.DampedSpring(dt=0.01), from the class itself."""
    from sda_amd.experiments import spring
    ch = spring.make_chain()
    A, b, Q, m0, P0 = (v.double().numpy() for v in (ch.A, ch.b, ch.Sigma_x, ch.mu_0, ch.Sigma_0))
    return A, b, np.linalg.cholesky(Q), m0, np.linalg.cholesky(P0)


def spring_observations(n_obs, step, sigma, burn, seed):
    """y (n_obs, 1) float32 of component 0 of one simulated trajectory, observation i at burn + (i + 1) step transitions."""
    A, b, Lq, m0, L0 = spring_matrices()
    rng = np.random.default_rng([seed, 77])
    x = m0 + L0 @ rng.standard_normal(4)
    y = []
    for i in range(burn + n_obs * step):
        x = A @ x + b + Lq @ rng.standard_normal(4)
        if i >= burn and (i - burn + 1) % step == 0:
            y.append(x[0] + sigma * rng.standard_normal())
    return np.asarray(y, np.float32)[:, None]


def spring_enks(y, members, step, sigma, burn, seed, lag=None, inflation=1.0):
    """The smoother in float64 numpy on the damped spring, component 0 observed: (members, (N - 1) step + 1, 4), the time
    convention of experiments.spring (the first returned state is the first observed one)."""
    A, b, Lq, m0, L0 = spring_matrices()
    rng = np.random.default_rng([seed, members])
    x = m0 + rng.standard_normal((members, 4)) @ L0.T
    for _ in range(burn):
        x = x @ A.T + b + rng.standard_normal((members, 4)) @ Lq.T
    n = len(y)
    S = np.empty((n * step + 1, members, 4))
    S[0] = x
    for i in range(n):
        t = (i + 1) * step
        for s in range(i * step + 1, t + 1):
            S[s] = S[s - 1] @ A.T + b + rng.standard_normal((members, 4)) @ Lq.T
        lo = 0 if lag is None else max(0, t - lag * step)
        S[:t + 1] = analysis(S[:t + 1], lo, t, [0], [0.0], [1.0], sigma, y[i], perturbations(members, 1, seed, i), inflation,
                             np.float64)[0]
    return S.transpose(1, 0, 2)[:, step:]


def moment_errors(x, mean, cov):
    """x (members, T + 1, d) against the exact posterior: (RMS of mean error / exact std, RMS relative error of the variances), each
    over all (time, component) entries."""
    var = np.diagonal(cov, axis1=-2, axis2=-1)
    em = (x.mean(axis=0) - mean) / np.sqrt(var)
    ev = (x.var(axis=0, ddof=1) - var) / var
    return float(np.sqrt((em ** 2).mean())), float(np.sqrt((ev ** 2).mean()))


# ---------------------------------------------------------------- the host twins (libsda_emu.so)
@functools.lru_cache(None)
def emu():
    from sda_amd import _lib, build
    lib = ctypes.CDLL(build.build_emu())
    P = ctypes.c_void_p
    lib.sda_enks_gain_host.restype = ctypes.c_int
    lib.sda_enks_gain_host.argtypes = [P, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(_lib.ChainObs), ctypes.c_float,
                                       ctypes.c_uint64, ctypes.c_int64, P, P, P, P]
    lib.sda_enks_update_host.restype = ctypes.c_int
    lib.sda_enks_update_host.argtypes = [P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, P, P]
    return lib


def host_obs(index, shift, scale, sigma, y):
    from sda_amd import _lib
    o = _lib.ChainObs()
    o.k = len(index)
    for i in range(min(o.k, _lib.CHAIN_MAXOBS)):
        o.idx[i], o.shift[i], o.scale[i] = index[i], shift[i], scale[i]
    o.sigma = sigma
    y = np.ascontiguousarray(y, np.float32)
    o.y = y.ctypes.data
    o._keep = y
    return o


def host_analysis(S, lo, t, index, shift, scale, sigma, y, seed, draw, inflation):
    """The two host twins on a copy of S: (S', a, z, status, (rc_gain, rc_update))."""
    S = np.array(S, dtype=np.float32)
    slabs, m, d = S.shape
    k = len(index)
    a, z, work = (np.full((max(k, 1), m), np.nan, np.float32) for _ in range(3))
    status = np.full(1, -1, np.int32)
    o = host_obs(index, shift, scale, sigma, y)
    lib = emu()
    rc1 = lib.sda_enks_gain_host(S[t].ctypes.data, m, d, d, ctypes.byref(o), inflation, seed, draw, a.ctypes.data, z.ctypes.data,
                                 work.ctypes.data, status.ctypes.data)
    rc2 = None
    if rc1 == 0:
        rc2 = lib.sda_enks_update_host(S[lo].ctypes.data, m * d, d, t - lo + 1, m, d, k, inflation, a.ctypes.data, z.ctypes.data)
    return S, a, z, int(status[0]), (rc1, rc2)
