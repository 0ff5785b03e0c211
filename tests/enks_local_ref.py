"""TEST-ONLY numpy replay of one analysis of the DOMAIN-LOCALISED ensemble Kalman smoother (include/sda_hip.h,
csrc/enks_local.hip) in a chosen dtype, with its own float64 plan builder (block centres, periodic distances, Gaspari-Cohn weights),
the cases the CPU and GPU tests share, and the ctypes binding of the host twins.  ``analysis(.., np.float64)`` is the reference; the
same call in float32 is the 'own error' of the project's bound rule (tests/chain_util.bound).  The window, inflation and
perturbation conventions, ``case`` (for the reduction to the global analysis) and the bound rule come from tests/enks_wide_ref.py
and tests/enks_ref.py by import."""
import ctypes
import functools

import numpy as np

from tests import enks_ref
from tests import enks_wide_ref

WINDOWS = enks_ref.WINDOWS
INFLATIONS = [1.0, 1.05]

#: (M, event, block, operator, radius, sigmas) -> the per-block list lengths it gives (``test_the_cases_cover_the_list_lengths``).
#: M covers {2, 15, 17, 67, 128}; the lists 0, 1, 3, 4, 5 and > 64 values (the matrix instruction contracts 4 at a time); the
#: blocks 1, 4, 32 (4 x 4 x 2), 45 (3 x 5 x 3: odd), 128 (one transform tile exactly) and 180 components (two tiles, the second
#: partly filled).  sigma = 1e-3 only where every block's listed anomalies have the full rank M - 1 (``full_rank``).
SHAPES = [
    (2, (1, 1, 8), (1, 1), 'stride2', 0.4, (1e-3, 1.0)),              # lists of 1 at the observed points, EMPTY between them
    (15, (1, 1, 40), (1, 4), 'stride2', 1.5, (1.0,)),                 # 3
    (17, (1, 1, 40), (1, 4), 'stride2', 2.0, (1.0,)),                 # 4
    (67, (1, 1, 40), (1, 4), 'stride2', 2.5, (1.0,)),                 # 5
    (128, (2, 16, 16), (4, 4), 'coarsen', 4.0, (1.0,)),               # > 64
    (15, (2, 16, 16), (4, 4), 'coarsen', 4.0, (1e-3, 1.0)),           # > 64, full rank
    (67, (2, 16, 16), (8, 8), 'satcoarsen', 2.0, (1.0,)),
    (17, (3, 12, 20), (3, 5), 'stride2', 3.0, (1.0,)),
    (128, (3, 12, 20), (6, 10), 'coarsen', 2.5, (1.0,)),
    (2, (2, 16, 16), (4, 4), 'stride2', 1.0, (1e-3, 1.0)),
]


# ---------------------------------------------------------------- the plan, float64
def gaspari_cohn(z):
    z = np.asarray(z, np.float64)
    out = np.zeros_like(z)
    a = z <= 1.0
    za = z[a]
    out[a] = -za ** 5 / 4 + za ** 4 / 2 + 5 * za ** 3 / 8 - 5 * za ** 2 / 3 + 1
    b = (z > 1.0) & (z < 2.0)
    zb = z[b]
    out[b] = zb ** 5 / 12 - zb ** 4 / 2 + 5 * zb ** 3 / 8 + 5 * zb ** 2 / 3 - 5 * zb + 4 - 2 / (3 * zb)
    return out


def plan(event, positions, radius, block):
    """dict(event, block, nblk, offsets, idx, rho (float64), comps): the CSR lists of every block in ascending i, an entry listed
    when its weight rounded to fp32 is strictly positive, and per block the flat indices of its components."""
    C, Hg, Wg = event
    bh, bw = block
    pos = np.asarray(positions, np.float64).reshape(-1, 2)
    offsets, idx, rho, comps = [0], [], [], []
    flat = np.arange(C * Hg * Wg).reshape(C, Hg, Wg)
    for br in range(Hg // bh):
        for bc in range(Wg // bw):
            rows, cols = np.arange(br * bh, (br + 1) * bh), np.arange(bc * bw, (bc + 1) * bw)
            centre = (rows.mean(), cols.mean())
            dr = np.abs(pos[:, 0] - centre[0]) % Hg
            dc = np.abs(pos[:, 1] - centre[1]) % Wg
            dist = np.hypot(np.minimum(dr, Hg - dr), np.minimum(dc, Wg - dc))
            w = gaspari_cohn(dist / radius)
            keep = np.nonzero(w.astype(np.float32) > 0)[0]
            idx.append(keep)
            rho.append(w[keep])
            offsets.append(offsets[-1] + len(keep))
            comps.append(flat[:, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].reshape(-1))
    return dict(event=event, block=block, nblk=len(comps), offsets=np.asarray(offsets, np.int32),
                idx=np.concatenate(idx).astype(np.int32), rho=np.concatenate(rho), comps=comps)


def plan32(event, positions, radius, block):
    """The same builder in float32 arithmetic: the 'own error' of the weights under the bound rule (same lists assumed)."""
    C, Hg, Wg = event
    bh, bw = block
    f = np.float32
    pos = np.asarray(positions, f).reshape(-1, 2)
    P = plan(event, positions, radius, block)
    rho = []
    b = 0
    for br in range(Hg // bh):
        for bc in range(Wg // bw):
            centre = (f(br * bh + (bh - 1) / 2), f(bc * bw + (bw - 1) / 2))
            i = P['idx'][P['offsets'][b]:P['offsets'][b + 1]]
            dr = np.abs(pos[i, 0] - centre[0]) % f(Hg)
            dc = np.abs(pos[i, 1] - centre[1]) % f(Wg)
            dist = np.sqrt(np.minimum(dr, f(Hg) - dr) ** 2 + np.minimum(dc, f(Wg) - dc) ** 2, dtype=f)
            z = dist / f(radius)
            za = np.minimum(z, f(1))
            zb = np.clip(z, f(1), f(2))
            near = -za ** 5 / f(4) + za ** 4 / f(2) + f(5) * za ** 3 / f(8) - f(5) * za ** 2 / f(3) + f(1)
            far = zb ** 5 / f(12) - zb ** 4 / f(2) + f(5) * zb ** 3 / f(8) + f(5) * zb ** 2 / f(3) - f(5) * zb + f(4) - f(2) / (f(3) * zb)
            rho.append(np.where(z <= 1, near, far).astype(f))
            b += 1
    return np.concatenate(rho)


def positions(name, event):
    """Hand-written (k, 2) positions of the case operators' outputs, flattened output order."""
    C, Hg, Wg = event
    if name == 'stride2':
        rows = [0.0] if Hg == 1 else [float(r) for r in range(0, Hg, 2)]
        return np.array([(r, float(c)) for _ in range(C) for r in rows for c in range(0, Wg, 2)])
    if name in ('coarsen', 'satcoarsen'):
        return np.array([(2 * i + 0.5, 2 * j + 0.5) for _ in range(C) for i in range(Hg // 2) for j in range(Wg // 2)])
    raise KeyError(name)


def operator(name, event):
    """A(x, dtype) for x (M, d) of that dtype -> (M, k), every operation in ``dtype``."""
    C, Hg, Wg = event

    def coarsen(x, dtype):
        c = x.reshape(-1, C, Hg // 2, 2, Wg // 2, 2)
        return ((c[:, :, :, 0, :, 0] + c[:, :, :, 0, :, 1] + c[:, :, :, 1, :, 0] + c[:, :, :, 1, :, 1]) * dtype(0.25)).reshape(len(x), -1)
    if name == 'stride2':
        if Hg == 1:
            return lambda x, dtype: x.reshape(-1, C, Wg)[:, :, ::2].reshape(len(x), -1)
        return lambda x, dtype: x.reshape(-1, C, Hg, Wg)[:, :, ::2, ::2].reshape(len(x), -1)
    if name == 'coarsen':
        return coarsen
    if name == 'satcoarsen':
        def A(x, dtype):
            c = coarsen(x, dtype)
            return c / (dtype(1) + np.abs(c))
        return A
    raise KeyError(name)


def device_operator(name, event):
    """The same operator through the package's own operators: (the ``observe`` operator, a callable on (M, d) device tensors)."""
    from sda_amd import observe
    C, Hg, Wg = event
    if name == 'stride2':
        op = observe.Subsample((slice(0, None, 2),)) if Hg == 1 else observe.Subsample.space(2)
    elif name == 'coarsen':
        op = observe.Coarsen(2)
    elif name == 'satcoarsen':
        op = observe.Compose(observe.Coarsen(2), observe.Pointwise('saturate'))
    else:
        raise KeyError(name)
    return op, (lambda x: op(x.reshape(-1, C, Hg, Wg)).reshape(x.shape[0], -1))


def full_rank(m, P):
    """Do the listed anomalies of EVERY non-empty block have the full rank M - 1 (see ``enks_wide_ref.full_rank``)?"""
    n = np.diff(P['offsets'])
    return bool((n[n > 0] >= m - 1).all())


def analysis(S, lo, t, A, sigma, y, eps, inflation, P, dtype):
    """One analysis on a copy of S (slabs, M, d) with the plan P: returns (S', H (M, k), W (nblk, M, M)) in `dtype`.  Every
    parameter is first rounded to float32, as the device receives it; so are the plan's weights."""
    S = np.array(S, dtype=dtype)
    m = S.shape[1]
    sigma = dtype(np.float32(sigma))
    lam = dtype(np.float32(inflation))
    y = np.asarray(y, np.float32).astype(dtype)
    eps = np.asarray(eps, np.float32).astype(dtype)
    if np.float32(inflation) != np.float32(1.0):
        S[t] = S[t] + (lam - dtype(1)) * (S[t] - S[t].mean(axis=0, dtype=dtype))
    H = np.asarray(A(S[t], dtype), dtype)
    Y = H - H.mean(axis=0, dtype=dtype)
    D = (y + sigma * eps) - H
    W = np.zeros((P['nblk'], m, m), dtype)
    off = P['offsets']
    for b in range(P['nblk']):
        i = P['idx'][off[b]:off[b + 1]]
        if not len(i):
            continue
        r = P['rho'][off[b]:off[b + 1]].astype(np.float32).astype(dtype)
        Yw = Y[:, i] * r
        G, B = Yw @ Y[:, i].T, Yw @ D[:, i].T
        W[b] = np.linalg.solve(G / dtype(m - 1) + sigma * sigma * np.eye(m, dtype=dtype), B / dtype(m - 1)).astype(dtype)
        comp = P['comps'][b]
        for s in range(lo, t + 1):
            xs = S[s][:, comp]
            S[s][:, comp] = xs + W[b].T @ (xs - xs.mean(axis=0, dtype=dtype))
    return S, H, W


@functools.lru_cache(None)
def case(m, event, block, name, radius, slabs, lo, t, inflation, sigma, seed=1234):
    """Inputs and both replays of one case, computed once and shared: dict(S, y, eps, A, P, ref64, ref32)."""
    d = int(np.prod(event))
    pos = positions(name, event)
    k = len(pos)
    rng = np.random.default_rng([seed, m, d, k, slabs])
    base = rng.standard_normal((m, d))
    S = (base[None] * np.linspace(0.5, 1.5, slabs)[:, None, None] + 0.5 * rng.standard_normal((slabs, m, d)) + 1.0).astype(np.float32)
    A = operator(name, event)
    y = (A(S[t].astype(np.float64), np.float64).mean(axis=0) + 0.3 * rng.standard_normal(k)).astype(np.float32)
    draw = 3
    eps = enks_ref.perturbations(m, k, seed, draw)
    P = plan(event, pos, radius, block)
    args = (S, lo, t, A, sigma, y, eps, inflation, P)
    out = dict(S=S, y=y, eps=eps, A=A, P=P, pos=pos, k=k, seed=seed, draw=draw, ref64=analysis(*args, np.float64),
               ref32=analysis(*args, np.float32))
    for v in (S, y, eps):
        v.setflags(write=False)
    return out


CASES = [(m, event, block, name, radius, w, lam, sig) for (m, event, block, name, radius, sigmas) in SHAPES for w in WINDOWS
         for lam in INFLATIONS for sig in sigmas]
IDS = [f'M{m}-{"x".join(map(str, e))}-b{"x".join(map(str, b))}-{name}-r{r}-w{w[0]}-lam{lam}-sig{sig}'
       for (m, e, b, name, r, w, lam, sig) in CASES]
SHAPE_IDS = [f'M{m}-{"x".join(map(str, e))}-b{"x".join(map(str, b))}-{name}-r{r}' for (m, e, b, name, r, _) in SHAPES]


# ---------------------------------------------------------------- the host twins (libsda_emu.so)
@functools.lru_cache(None)
def emu():
    lib = enks_wide_ref.emu()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = {
        'sda_enkl_pack_host': [P, P, I, I, P],
        'sda_enkl_weights_host': [P, I, I, P, P, P, I, F, P, P, P],
        'sda_enkl_transform_host': [P, L, L, I, I, I, I, I, I, I, P, P],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I, args
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


def host_csr(P):
    """The plan as the device receives it: (offsets int32, idx int32, rho float32), C-contiguous (idx / rho never empty arrays)."""
    idx = np.ascontiguousarray(P['idx'], np.int32) if len(P['idx']) else np.zeros(1, np.int32)
    rho = np.ascontiguousarray(P['rho'], np.float32) if len(P['rho']) else np.zeros(1, np.float32)
    return np.ascontiguousarray(P['offsets'], np.int32), idx, rho


def host_weights(P, H, y, sigma, seed, draw, eps_in=None, Y=None, D=None):
    """Prepare (enks_wide's twin), pack and the per-block solve by the host twins: dict(Y, D, eps, T, W, status, rcs).  With Y and
    D given, prepare is skipped (the device's own Y, D)."""
    lib = emu()
    rcs = []
    if Y is None:
        H = np.ascontiguousarray(H, np.float32)
        m, k = H.shape
        y = np.ascontiguousarray(y, np.float32)
        Y, D, eps = (np.full((m, k), np.nan, np.float32) for _ in range(3))
        eps_in = None if eps_in is None else np.ascontiguousarray(eps_in, np.float32)
        rcs.append(lib.sda_enkw_prepare_host(_p(H), m, k, _p(y), sigma, seed, draw, _p(Y), _p(D), _p(eps), _p(eps_in)))
    else:
        Y, D, eps = np.ascontiguousarray(Y, np.float32), np.ascontiguousarray(D, np.float32), None
        m, k = Y.shape
    T = np.full((k, 2 * m), np.nan, np.float32)
    W = np.full((P['nblk'], m, m), np.nan, np.float32)
    status = np.full(P['nblk'], -1, np.int32)
    work = np.empty(P['nblk'] * m * m)
    offsets, idx, rho = host_csr(P)
    rcs.append(lib.sda_enkl_pack_host(_p(Y), _p(D), m, k, _p(T)))
    rcs.append(lib.sda_enkl_weights_host(_p(T), m, k, _p(offsets), _p(idx), _p(rho), P['nblk'], sigma, _p(work), _p(W), _p(status)))
    return dict(Y=Y, D=D, eps=eps, T=T, W=W, status=status, rcs=tuple(rcs))


def host_transform(P, S, lo, t, W):
    """The localised update on slabs lo .. t of S (slabs, M, d) float32 C-contiguous, in place: the return code."""
    slabs, m, d = S.shape
    W = np.ascontiguousarray(W, np.float32)
    offsets = np.ascontiguousarray(P['offsets'], np.int32)
    C, Hg, Wg = P['event']
    return emu().sda_enkl_transform_host(S[lo].ctypes.data, m * d, d, t - lo + 1, m, C, Hg, Wg, P['block'][0], P['block'][1],
                                         _p(offsets), _p(W))


def host_analysis(c, lo, t, sigma, inflation, *, y=None, eps_in=None):
    """The host twins on a copy of the case's ensemble, H by the float32 numpy operator: (S', H, host_weights dict)."""
    S = np.array(c['S'], dtype=np.float32)
    assert enks_wide_ref.host_inflate(S, t, inflation) == 0
    H = np.ascontiguousarray(c['A'](S[t], np.float32), np.float32)
    w = host_weights(c['P'], H, c['y'] if y is None else y, sigma, c['seed'], c['draw'], eps_in)
    if w['rcs'] == (0, 0, 0):
        assert host_transform(c['P'], S, lo, t, w['W']) == 0
    return S, H, w


def acting(W, sigma):
    """What of W (nblk, M, M) is compared.  At sigma = 1 W itself.  At sigma = 1e-3 its part orthogonal to the all-ones vector
    along the summed member axis: the update multiplies CENTRED values, so only that part acts, and the all-ones direction, whose
    eigenvalue is sigma^2 in every block, carries an fp32-replay error of 2^-24 / sigma^2 that would make the bound of W vacuous
    (``enks_wide_ref.full_rank`` has the same remark for S)."""
    W = np.asarray(W, np.float64)
    return W if sigma == 1.0 else W - W.mean(axis=-2, keepdims=True)


def blocks_listing(P, i):
    """The blocks whose list contains observed value i."""
    off = P['offsets']
    return [b for b in range(P['nblk']) if i in P['idx'][off[b]:off[b + 1]]]
