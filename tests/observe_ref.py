"""A float64 numpy reference of the observation operators, written from their definitions (not from the kernels).

Every linear operator is an explicit sparse map: a list of terms ``(out_index, in_index, weight)``, where the two index arrays
are flat positions in the row-major output and input.  The forward is ``out[oi] += w * x[ii]`` and the adjoint is the
transpose of that same list, ``gx[ii] += w * r[oi]`` (a scatter-add), so forward and adjoint cannot disagree.  The index
arrays come from numpy's own slicing / modular arithmetic applied to ``arange`` grids of coordinates:

    subsample  x[..., s_k]                      numpy slicing of the grid of flat input positions
    select     x.select(dim, index)             the same, one index along one axis
    coarsen    mean over f x f cells            out (Y, X) <- in (Y f + a, X f + b), weight 1 / f^2, a, b < f
    vorticity  d_x u - d_y v, periodic central  out (y, x) <- +u(y, x+1)/2 - u(y, x-1)/2 - v(y+1, x)/2 + v(y-1, x)/2  (mod w, h)
    mask       x * m, m against the trailing dims  (numpy broadcasting of the weight)
    timediff   x.select(dim, i) - x.select(dim, j)

Non-linear members (pointwise) carry ``f`` and ``df`` in float64; a chain is a list of members."""
import numpy as np


def _grid(shape):
    """Flat row-major positions of an array of this shape, shaped like it."""
    n = int(np.prod(shape, dtype=np.int64))
    return np.arange(n, dtype=np.int64).reshape(shape)


class LinearMap:
    """``terms``: list of (oi, ii, w) with oi, ii int64 arrays of equal length and w a float or an array of that length.
    Within one term no output position and no input position occurs twice (each term is a one-to-one pairing; sums arise
    across terms), so ``a[idx] += v`` is a true scatter-add.  Small maps verify that on construction."""

    def __init__(self, in_shape, out_shape, terms):
        self.in_shape, self.out_shape = tuple(in_shape), tuple(out_shape)
        self.terms = []
        for oi, ii, w in terms:
            oi, ii = np.asarray(oi, np.int64).reshape(-1), np.asarray(ii, np.int64).reshape(-1)
            w = np.asarray(w, np.float64).reshape(-1) if np.ndim(w) else float(w)
            assert oi.size == ii.size
            if oi.size <= 1 << 16:
                assert np.unique(oi).size == oi.size and np.unique(ii).size == ii.size
            self.terms.append((oi, ii, w))

    def forward(self, x):
        x = np.asarray(x, np.float64).reshape(-1)
        out = np.zeros(int(np.prod(self.out_shape, dtype=np.int64)))
        for oi, ii, w in self.terms:
            out[oi] += w * x[ii]
        return out.reshape(self.out_shape)

    def adjoint(self, r):
        r = np.asarray(r, np.float64).reshape(-1)
        gx = np.zeros(int(np.prod(self.in_shape, dtype=np.int64)))
        for oi, ii, w in self.terms:
            gx[ii] += w * r[oi]
        return gx.reshape(self.in_shape)

    # a linear map is its own linearisation
    def linearize(self, x):
        return self.forward(x), self.adjoint


def subsample(in_shape, slices):
    """x[..., s_k] with one slice per trailing dim."""
    key = (Ellipsis,) + tuple(slices) if len(slices) else (Ellipsis,)
    ii = _grid(in_shape)[key]
    return LinearMap(in_shape, ii.shape, [(_grid(ii.shape), ii, 1.0)])


def select(in_shape, dim, index):
    ii = np.take(_grid(in_shape), index, axis=dim)
    return LinearMap(in_shape, ii.shape, [(_grid(ii.shape), ii, 1.0)])


def coarsen(in_shape, f):
    *lead, h, w = in_shape
    out_shape = (*lead, h // f, w // f)
    g = _grid(in_shape)
    oi = _grid(out_shape)
    terms = []
    for a in range(f):
        for b in range(f):
            terms.append((oi, g[..., a::f, b::f][..., :h // f, :w // f], 1.0 / (f * f)))
    return LinearMap(in_shape, out_shape, terms)


def vorticity(in_shape):
    *lead, two, h, w = in_shape
    assert two == 2
    out_shape = (*lead, h, w)
    g = _grid(in_shape)
    u, v = g[..., 0, :, :], g[..., 1, :, :]
    xs, ys = np.arange(w), np.arange(h)
    oi = _grid(out_shape)
    terms = [(oi, u[..., :, (xs + 1) % w], 0.5), (oi, u[..., :, (xs - 1) % w], -0.5),
             (oi, v[..., (ys + 1) % h, :], -0.5), (oi, v[..., (ys - 1) % h, :], 0.5)]
    return LinearMap(in_shape, out_shape, terms)


def mask(in_shape, m):
    g = _grid(in_shape)
    wgt = np.broadcast_to(np.asarray(m, np.float64), in_shape)
    return LinearMap(in_shape, in_shape, [(g, g, np.ascontiguousarray(wgt).reshape(-1))])


def timediff(in_shape, dim, i, j):
    g = _grid(in_shape)
    gi, gj = np.take(g, i, axis=dim), np.take(g, j, axis=dim)
    oi = _grid(gi.shape)
    return LinearMap(in_shape, gi.shape, [(oi, gi, 1.0), (oi, gj, -1.0)])


_PW = {
    'saturate': (lambda v: v / (1.0 + np.abs(v)), lambda v: 1.0 / (1.0 + np.abs(v)) ** 2),
    'tanh': (np.tanh, lambda v: 1.0 - np.tanh(v) ** 2),
    'square': (lambda v: v * v, lambda v: 2.0 * v),
    'abs': (np.abs, np.sign),
}


class Pointwise:
    def __init__(self, in_shape, kind):
        self.in_shape = self.out_shape = tuple(in_shape)
        self.f, self.df = _PW[kind]

    def forward(self, x):
        with np.errstate(over='ignore'):
            return self.f(np.asarray(x, np.float64))

    def linearize(self, x):
        x = np.asarray(x, np.float64)
        with np.errstate(over='ignore'):
            d = self.df(x)
        return self.forward(x), (lambda r: np.asarray(r, np.float64).reshape(x.shape) * d)


class Chain:
    """members applied left to right; ``build`` entries are callables ``in_shape -> member``."""

    def __init__(self, in_shape, *build):
        self.in_shape = tuple(in_shape)
        self.members = []
        shape = self.in_shape
        for b in build:
            m = b(shape)
            self.members.append(m)
            shape = m.out_shape
        self.out_shape = shape

    def forward(self, x):
        for m in self.members:
            x = m.forward(x)
        return x

    def linearize(self, x):
        vjps = []
        for m in self.members:
            x, v = m.linearize(x)
            vjps.append(v)

        def vjp(r):
            for v in reversed(vjps):
                r = v(r)
            return r
        return x, vjp

    def adjoint(self, r):
        for m in reversed(self.members):
            r = m.adjoint(r)
        return r


def gaussian_guidance(A, x, eps, y, std, gamma, mu, sigma):
    """A^T((y - A((x - sigma eps)/mu)) / (std^2 + gamma (sigma/mu)^2)) for a linear A; y broadcasts against A(x) as numpy
    broadcasts.  A is linear, so A((x - sigma eps)/mu) is formed as (A x - sigma A eps)/mu on the observed positions."""
    y = np.asarray(y, np.float64)
    axhat = (A.forward(x) - sigma * A.forward(eps)) / mu
    var = std ** 2 + gamma * (sigma / mu) ** 2
    return A.adjoint((y - axhat) / var)


# ------------------------------------------------------------------ dense forms for tensors too large for index lists
# The same definitions written with numpy slicing / modular index vectors on the array itself; they keep the input's dtype
# (float32 in, float32 arithmetic out), and tests/test_observe_ref_host.py checks each against its LinearMap in float64.
def _key(slices):
    return (Ellipsis,) + tuple(slices)


def subsample_dense(x, slices):
    return np.ascontiguousarray(np.asarray(x)[_key(slices)])


def subsample_adjoint_dense(r, in_shape, slices):
    r = np.asarray(r)
    gx = np.zeros(in_shape, r.dtype)
    gx[_key(slices)] = r
    return gx


def coarsen_adjoint_dense(r, f):
    r = np.asarray(r)
    return np.repeat(np.repeat(r, f, axis=-2), f, axis=-1) * r.dtype.type(1.0 / (f * f))


def vorticity_dense(x):
    x = np.asarray(x)
    h, w = x.shape[-2:]
    xs, ys = np.arange(w), np.arange(h)
    u, v = x[..., 0, :, :], x[..., 1, :, :]
    half = x.dtype.type(0.5)
    return (u[..., :, (xs + 1) % w] - u[..., :, (xs - 1) % w]) * half - (v[..., (ys + 1) % h, :] - v[..., (ys - 1) % h, :]) * half


def vorticity_adjoint_dense(r):
    """Transpose of vorticity_dense: u(y, x) enters out(y, x-1) with +1/2 and out(y, x+1) with -1/2; v(y, x) enters
    out(y-1, x) with -1/2 and out(y+1, x) with +1/2."""
    r = np.asarray(r)
    h, w = r.shape[-2:]
    xs, ys = np.arange(w), np.arange(h)
    half = r.dtype.type(0.5)
    gu = (r[..., :, (xs - 1) % w] - r[..., :, (xs + 1) % w]) * half
    gv = (r[..., (ys + 1) % h, :] - r[..., (ys - 1) % h, :]) * half
    return np.stack([gu, gv], axis=-3)


def timediff_dense(x, dim, i, j):
    x = np.asarray(x)
    return np.take(x, i, axis=dim) - np.take(x, j, axis=dim)


def timediff_adjoint_dense(r, in_shape, dim, i, j):
    r = np.asarray(r)
    gx = np.zeros(in_shape, r.dtype)
    idx = [slice(None)] * len(in_shape)
    idx[dim] = i
    gx[tuple(idx)] += r
    idx[dim] = j
    gx[tuple(idx)] -= r
    return gx
