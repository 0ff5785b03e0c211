"""TEST-ONLY numpy replay of one analysis of the ensemble Kalman smoother in its ENSEMBLE-space form (include/sda_hip.h,
csrc/enks_wide.hip) in a chosen dtype, the observation operators of the cases as dtype-generic numpy, the cases the CPU and GPU
tests share, and the ctypes binding of the host twins.  ``analysis(.., np.float64)`` is the reference; the same call in float32 is
the 'own error' of the project's bound rule (tests/chain_util.bound).  tests/test_enks_wide_host.py pins the float64 replay to
``tests/enks_ref.analysis`` (the observation-space form, which this change did not write) on every case whose operator is a
component selection."""
import ctypes
import functools

import numpy as np

from tests import enks_ref

WINDOWS = enks_ref.WINDOWS
INFLATIONS = [1.0, 1.05]
SIGMAS = [1e-3, 1.0]
KC = 512                                                              # ENKW_KC: observed values per Gram chunk

#: (M, d, k, operator).  M covers {2, 15, 17, 67, 128}, d {1, 48, 200, 2 16 16}, k {1, 5, 300, 517}; 517 crosses a Gram chunk and
#: is no multiple of 4.  'select' observes components (arange(k) * 7) % d with a varying shift and scale, 'vortcoarse' is
#: Coarsen(2) of Vorticity on the (2, 16, 16) state (k = 64), 'saturate' is Pointwise('saturate') of every component (k = d).
SHAPES = [(2, 1, 1, 'select'), (15, 48, 5, 'select'), (15, 48, 300, 'select'), (17, 200, 300, 'select'), (67, 512, 517, 'select'),
          (128, 48, 300, 'select'), (128, 200, 300, 'select'), (128, 512, 64, 'vortcoarse'), (67, 200, 200, 'saturate')]


def full_rank(m, d, k, name):
    """Do the anomalies Y (M, k) have the full rank M - 1?  Where they do not, Y Y^T / (M - 1) + sigma^2 I has eigenvalues sigma^2
    beside eigenvalues of order 1, and an all-float32 replay of the M x M solve is off by about 2^-24 / sigma^2 of W in those
    directions: 0.06 at sigma = 1e-3 (measured: a bound of 0.39 on values of order 1 at (15, 48, 5)), which would make the bound
    vacuous.  (The kernels keep steps 2 - 4 in float64 for exactly that reason.)  Those shapes are therefore paired with sigma = 1
    only; the direction of the all-ones vector, whose eigenvalue is sigma^2 in every case, is harmless because step 5 multiplies
    centred values."""
    distinct = min(k, d) if name == 'select' else k
    return distinct >= m - 1


def shared(m, d, k, name):
    """Is the shape one that the observation-space smoother serves as well (csrc/enks.hip: d <= 64, k <= 64, a component selection)?
    On those the float64 replay here is held to ``enks_ref.analysis``.  Past them that replay is no yardstick at 1e-9: at
    k = 300 and M = 15 or 17 its 300 x 300 float64 solve has rank 14 or 16 beside sigma^2 = 1e-6, and against an 80-bit replay it is
    itself off by 5.0e-9 .. 9.1e-9 (1e-9 max|S| is 5.6e-9 .. 7.7e-9) where the replay here is off by less than 1e-14."""
    return name == 'select' and d <= 64 and k <= 64


def selection(d, k):
    index = [(7 * i) % d for i in range(k)]
    shift = [0.1 * (i % 7) for i in range(k)]
    scale = [1.0 + 0.25 * (i % 5) for i in range(k)]
    return index, shift, scale


def operator(name, d, k):
    """A(x, dtype) for x (M, d) of that dtype -> (M, k), every operation in ``dtype``."""
    if name == 'select':
        index, shift, scale = selection(d, k)
        return lambda x, dtype: enks_ref.obs_apply(x, index, shift, scale, dtype)
    if name == 'saturate':
        assert k == d
        return lambda x, dtype: x / (dtype(1) + np.abs(x))
    if name == 'vortcoarse':
        assert (d, k) == (512, 64)

        def A(x, dtype):
            f = x.reshape(-1, 2, 16, 16)
            u, v = f[:, 0], f[:, 1]
            half = dtype(0.5)
            w = half * np.roll(u, -1, -1) - half * np.roll(u, 1, -1) - half * np.roll(v, -1, -2) + half * np.roll(v, 1, -2)
            c = w.reshape(-1, 8, 2, 8, 2)
            return ((c[:, :, 0, :, 0] + c[:, :, 0, :, 1] + c[:, :, 1, :, 0] + c[:, :, 1, :, 1]) * dtype(0.25)).reshape(-1, 64)
        return A
    raise KeyError(name)


def device_operator(name, d, k):
    """The same operator on (M, d) device tensors, through the package's own operators."""
    import torch
    from sda_amd import observe
    if name == 'select':
        index, shift, scale = selection(d, k)

        def A(x):
            idx = torch.tensor(index, device=x.device)
            return (x[..., idx] - torch.tensor(shift, device=x.device)) / torch.tensor(scale, device=x.device)
        return A
    if name == 'saturate':
        return observe.Pointwise('saturate')
    if name == 'vortcoarse':
        vort, coarse = observe.Vorticity(), observe.Coarsen(2)
        return lambda x: coarse(vort(x.reshape(-1, 2, 16, 16))).reshape(x.shape[0], 64)
    raise KeyError(name)


def analysis(S, lo, t, A, sigma, y, eps, inflation, dtype):
    """One analysis on a copy of S (slabs, M, d): returns (S', H (M, k), W (M, M)) in `dtype`.  Every parameter is first rounded to
    float32, as the device receives it."""
    S = np.array(S, dtype=dtype)
    m = S.shape[1]
    sigma = dtype(np.float32(sigma))
    lam = dtype(np.float32(inflation))
    y = np.asarray(y, np.float32).astype(dtype)
    eps = np.asarray(eps, np.float32).astype(dtype)
    if np.float32(inflation) != np.float32(1.0):                      # step 1
        S[t] = S[t] + (lam - dtype(1)) * (S[t] - S[t].mean(axis=0, dtype=dtype))
    H = np.asarray(A(S[t], dtype), dtype)                             # step 2
    Y = H - H.mean(axis=0, dtype=dtype)
    D = (y + sigma * eps) - H
    G, B = Y @ Y.T, Y @ D.T                                           # step 3
    W = np.linalg.solve(G / dtype(m - 1) + sigma * sigma * np.eye(m, dtype=dtype), B / dtype(m - 1)).astype(dtype)      # step 4
    for s in range(lo, t + 1):                                        # step 5
        xs = S[s]
        S[s] = xs + W.T @ (xs - xs.mean(axis=0, dtype=dtype))
    return S, H, W


@functools.lru_cache(None)
def case(m, d, k, name, slabs, lo, t, inflation, sigma, seed=1234):
    """Inputs and both replays of one case, computed once and shared: dict(S, y, eps, A, ref64, ref32)."""
    rng = np.random.default_rng([seed, m, d, k, slabs])
    base = rng.standard_normal((m, d))
    S = (base[None] * np.linspace(0.5, 1.5, slabs)[:, None, None] + 0.5 * rng.standard_normal((slabs, m, d)) + 1.0).astype(np.float32)
    A = operator(name, d, k)
    y = (A(S[t].astype(np.float64), np.float64).mean(axis=0) + 0.3 * rng.standard_normal(k)).astype(np.float32)
    draw = 3
    eps = enks_ref.perturbations(m, k, seed, draw)
    args = (S, lo, t, A, sigma, y, eps, inflation)
    out = dict(S=S, y=y, eps=eps, A=A, seed=seed, draw=draw, ref64=analysis(*args, np.float64), ref32=analysis(*args, np.float32))
    for v in (S, y, eps):
        v.setflags(write=False)
    return out


CASES = [(m, d, k, name, w, lam, sig) for (m, d, k, name) in SHAPES for w in WINDOWS for lam in INFLATIONS for sig in SIGMAS
         if sig == 1.0 or full_rank(m, d, k, name)]


# ---------------------------------------------------------------- the host twins (libsda_emu.so)
@functools.lru_cache(None)
def emu():
    from sda_amd import build
    lib = ctypes.CDLL(build.build_emu())
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = {
        'sda_enkw_prepare_host': [P, I, I, P, F, ctypes.c_uint64, L, P, P, P, P],
        'sda_enkw_gram_host': [P, P, I, I, P],
        'sda_enkw_solve_host': [P, I, I, F, P, P, P],
        'sda_enkw_transform_host': [P, L, L, I, I, L, P, F, I],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I, args
    lib.sda_enkw_gram_doubles.restype, lib.sda_enkw_gram_doubles.argtypes = L, [I, I]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


def host_inflate(S, t, inflation):
    """Step 1 on slab t of S (slabs, M, d) float32 C-contiguous, in place: the return code."""
    slabs, m, d = S.shape
    return emu().sda_enkw_transform_host(S[t].ctypes.data, m * d, d, 1, m, d, None, inflation, 1)


def host_weights(H, y, sigma, seed, draw, eps_in=None):
    """Steps 2 - 4 by the host twins: dict(Y, D, eps, part, W, status, rcs)."""
    H = np.ascontiguousarray(H, np.float32)
    m, k = H.shape
    lib = emu()
    y = np.ascontiguousarray(y, np.float32)
    Y, D, eps = (np.full((m, k), np.nan, np.float32) for _ in range(3))
    W = np.full((m, m), np.nan, np.float32)
    status = np.full(1, -1, np.int32)
    out = dict(Y=Y, D=D, eps=eps, part=None, W=W, status=status)
    eps_in = None if eps_in is None else np.ascontiguousarray(eps_in, np.float32)
    rcs = [lib.sda_enkw_prepare_host(_p(H), m, k, _p(y), sigma, seed, draw, _p(Y), _p(D), _p(eps), _p(eps_in))]
    if rcs[0] == 0:
        part = out['part'] = np.full(lib.sda_enkw_gram_doubles(m, k), np.nan)
        work = np.empty(m * m)
        rcs.append(lib.sda_enkw_gram_host(_p(Y), _p(D), m, k, _p(part)))
        rcs.append(lib.sda_enkw_solve_host(_p(part), m, k, sigma, _p(work), _p(W), _p(status)))
    out['rcs'] = tuple(rcs)
    return out


def host_transform(S, lo, t, W):
    """Step 5 on slabs lo .. t of S (slabs, M, d) float32 C-contiguous, in place: the return code."""
    slabs, m, d = S.shape
    W = np.ascontiguousarray(W, np.float32)
    return emu().sda_enkw_transform_host(S[lo].ctypes.data, m * d, d, t - lo + 1, m, d, _p(W), 1.0, 0)


def host_analysis(c, lo, t, sigma, inflation, *, y=None, eps_in=None):
    """The host twins on a copy of the case's ensemble, H by the float32 numpy operator: (S', H, host_weights dict)."""
    S = np.array(c['S'], dtype=np.float32)
    assert host_inflate(S, t, inflation) == 0
    H = np.ascontiguousarray(c['A'](S[t], np.float32), np.float32)
    w = host_weights(H, c['y'] if y is None else y, sigma, c['seed'], c['draw'], eps_in)
    if w['rcs'] == (0, 0, 0):
        assert host_transform(S, lo, t, w['W']) == 0
    return S, H, w
