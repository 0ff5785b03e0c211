"""NumPy restatement of the adjoint of the Kolmogorov flow's explicit terms, written the way ``kflow_explicit_vjp_kernel``
(sda_amd/csrc/kflow.hip) is: phase A gives every face its cotangent and the five partials of its flux, phase B gathers per cell and
per face role (the cell as the cm, c0, cp, cpp tap of four faces along each axis, and inside the advecting velocity of two faces).
dtype-parametrised through the ``kflow_ref.Flow`` it is handed, and the torch-autograd oracles every VJP test compares with.

Derivative conventions (those of torch autograd on ``chains._kflow_flux``): ``a > 0`` selects the upwind branch and ``a == 0`` the
else branch, the selection itself carries no derivative; ``d == 0`` gives ``r = 0`` with zero derivative; ``|r|`` has derivative
``sign(r)``, 0 at ``r == 0``.
"""
import numpy as np
import torch

from sda_amd import chains
from tests import kflow_ref as R


def _s(a, di, dj):
    """a[i + di, j + dj], periodic."""
    return np.roll(a, (-di, -dj), (-2, -1))


def flux_partials(flow, a, cm, c0, cp, cpp, lam):
    """lam x the partials of ``Flow.flux`` with respect to (cm, c0, cp, cpp, a), per face."""
    T = flow.dtype
    C = a * flow.dh
    d = cp - c0
    pos = a > 0
    low = np.where(pos, c0, cp)
    num = np.where(pos, c0 - cm, cpp - cp)
    dhl = np.where(pos, T(0.5) * (T(1) - C), -T(0.5) * (T(1) + C))
    hl = dhl * d
    nz = d != 0
    safe = np.where(nz, d, T(1))
    inv = np.where(nz, T(1) / safe, T(0))
    r = np.where(nz, num / safe, T(0))
    ar = np.abs(r)
    s = np.sign(r).astype(T)
    q1 = T(1) / (T(1) + ar)
    phi = (r + ar) * q1
    dphi = ((T(1) + s) - phi * s) * q1
    gn = (hl * dphi) * inv
    gd = phi * dhl - gn * r
    la = lam * a
    zero = np.zeros_like(la)
    return (np.where(pos, -la * gn, zero),
            np.where(pos, la * ((T(1) + gn) - gd), -la * gd),
            np.where(pos, la * gd, la * ((T(1) + gd) - gn)),
            np.where(pos, zero, la * gn),
            lam * ((low + phi * hl) - a * (phi * (T(0.5) * flow.dh * d))))


def explicit_vjp(flow, x, g):
    """(d Flow.explicit / dx at x)^T g in flow.dtype; x, g (..., 2, N, N)."""
    T = flow.dtype
    x, g = np.asarray(x, dtype=T), np.asarray(g, dtype=T)
    u, v = x[..., 0, :, :], x[..., 1, :, :]
    gU, gV = g[..., 0, :, :], g[..., 1, :, :]
    half = T(0.5)

    def faces(c, a, gc, axis):
        di, dj = (1, 0) if axis == 0 else (0, 1)
        lam = -flow.dh * (gc - _s(gc, di, dj))
        return flux_partials(flow, a, _s(c, -di, -dj), c, _s(c, di, dj), _s(c, 2 * di, 2 * dj), lam)

    xu = faces(u, half * (u + _s(u, 1, 0)), gU, 0)
    yu = faces(u, half * (v + _s(v, 1, 0)), gU, 1)
    xv = faces(v, half * (u + _s(u, 0, 1)), gV, 0)
    yv = faces(v, half * (v + _s(v, 0, 1)), gV, 1)

    def taps(w, axis):
        di, dj = (1, 0) if axis == 0 else (0, 1)
        # the cell is cm of the next face, c0 of its own, cp of the previous one and cpp of the one before that
        return (_s(w[0], di, dj) + w[1]) + (_s(w[2], -di, -dj) + _s(w[3], -2 * di, -2 * dj))

    def lin(gc):
        return gc + flow.delta * (flow.nu * flow.lap(gc) - T(0.1) * gc)

    gu = lin(gU)
    gu = gu + taps(xu, 0)
    gu = gu + taps(yu, 1)
    gu = gu + half * ((xu[4] + _s(xu[4], -1, 0)) + (xv[4] + _s(xv[4], 0, -1)))
    gv = lin(gV)
    gv = gv + taps(xv, 0)
    gv = gv + taps(yv, 1)
    gv = gv + half * ((yu[4] + _s(yu[4], -1, 0)) + (yv[4] + _s(yv[4], 0, -1)))
    return np.stack((gu, gv), axis=-3)


# ---------------------------------------------------------------- torch-autograd oracles (the torch route on the CPU, as it stands)
def autograd_vjp(fn, x, g, dtype):
    """(d fn / dx at x)^T g by torch autograd on the CPU in `dtype`; x, g NumPy arrays, returns a NumPy array of `dtype`."""
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_()
    y = fn(xt)
    out, = torch.autograd.grad(y, xt, torch.from_numpy(np.asarray(g)).to(dtype).reshape(y.shape))
    return out.numpy()


def oracles(fn, x, g):
    """(float32 oracle, float64 oracle) of the VJP of `fn`."""
    return autograd_vjp(fn, x, g, torch.float32), autograd_vjp(fn, x, g, torch.float64)


def chain_for(n, dt=0.2, steps=None):
    """The torch-route chain of size n; `steps` overrides the sub-step count (delta as kflow_ref.Flow(n, dt) has it)."""
    chain = chains.KolmogorovFlow(size=n, dt=dt)
    if steps is not None:
        chain.steps = steps
    return chain


def prior_field(n, seed, batch=()):
    z = np.random.default_rng(seed).standard_normal((*batch, 2, n, n))
    return R.Flow(n, 0.2).prior(z).astype(np.float32)


def cotangent(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def bound_and_own(ref32, ref64):
    """``kflow_ref.bound`` plus the condition on the inputs: the oracle's own float32 error must be small against the result, or a
    near-tie made the two precisions take different branches of the limiter and the case says nothing."""
    b, own = R.bound(ref32, ref64)
    assert own <= 1e-4 * float(np.abs(ref64).max()), ('the inputs sit on a tie of the limiter', own, float(np.abs(ref64).max()))
    return b, own
