"""TEST-ONLY helpers shared by tests/test_chains_vjp_host.py and tests/test_gpu_chains_vjp.py: the ctypes binding of the adjoint's
host replay (libsda_emu.so), the oracle -- torch autograd through the torch-ops ``rk4`` of sda_amd/chains.py on the CPU, in float64
with its float32 run as the yardstick -- and the check that prints its figures.

Tolerance: ``chain_util.bound`` = max(1e-6 max|ref64|, 3 |torch-route fp32 - torch-route fp64|), one number per array.  Every
case also requires of its INPUTS that this bound stays below 1e-3 max|ref64|: a trajectory long enough for chaos to inflate the
oracle's own error would leave a test that cannot fail."""
import ctypes
import functools

import numpy as np
import torch

from sda_amd import _lib, chains
from tests import chain_util as U
from tests import philox_ref

P = ctypes.c_void_p
#: the chains of the fixture plus the sub-stepped ones the recompute schedule needs
CHAINS = dict(U.CHAINS)
CHAINS['l63_s3'] = ('Lorenz63', {'dt': 0.03, 'steps': 3})
CHAINS['l96_5_s3'] = ('Lorenz96', {'n': 5, 'dt': 0.03, 'steps': 3})
CHAINS['lv_s3'] = ('LotkaVolterra', {'dt': 0.03, 'steps': 3})


def make(key, **kw):
    cls, args = CHAINS[key]
    return getattr(chains, cls)(**args, **kw)


def x0_of(key):
    """The fixture's initial states of the chain's family, (7, d) fp32."""
    base = {'l63_s3': 'l63', 'l96_5_s3': 'l96_5', 'lv_s3': 'lv'}.get(key, key)
    return U.golden()[f'{base}/x0']


def cotangent(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(None)
def emu():
    lib = U.emu()
    sig = {
        'sda_chain_advance_vjp_host': [ctypes.POINTER(_lib.ChainVjp)],
        'sda_chain_log_prob_grad_host': [ctypes.POINTER(_lib.ChainModel), P, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, P, P],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, args
    return lib


def emu_vjp(chain, x_in, states, g, transitions, every, *, pad=0, anc=None, rc_only=False):
    """Host replay of sda_chain_advance_vjp.  x_in (m, d), states (>= transitions - 1, m, d) or None, g (transitions, m, d) or
    (m, d), all fp32.  pad > 0 lays every array out with a particle stride of d + pad floats (the gaps hold 7 and must survive)."""
    model = chain.model()
    m, d = x_in.shape
    sp = d + pad

    def lay(a):
        if a is None:
            return None
        big = np.full(a.shape[:-1] + (sp,), 7.0, np.float32)
        big[..., :d] = a
        return big

    xb, sb, gb = lay(x_in), lay(states), lay(g)
    gx = np.full((m, sp), 7.0, np.float32)
    a = _lib.ChainVjp()
    a.model = model
    a.x_in, a.in_sp = xb.ctypes.data, sp
    a.anc = None if anc is None else anc.ctypes.data
    if sb is not None:
        a.states, a.st_st, a.st_sp = sb.ctypes.data, m * sp, sp
    a.g, a.g_st, a.g_sp = gb.ctypes.data, m * sp, sp
    a.every, a.m, a.transitions = int(every), m, transitions
    a.gx, a.gx_sp = gx.ctypes.data, sp
    rc = emu().sda_chain_advance_vjp_host(ctypes.byref(a))
    if rc_only:
        return rc
    assert rc == 0, f'sda_chain_advance_vjp_host rc={rc}'
    assert np.all(gx[:, d:] == 7.0)
    return np.ascontiguousarray(gx[:, :d])


def emu_log_prob_grad(chain, x):
    """Host replay of sda_chain_log_prob_grad on (b, L, d) fp32 -> (value (b,) float64, grad (b, L, d) fp32)."""
    model = chain.model()
    x = np.ascontiguousarray(x, np.float32)
    b, L, d = x.shape
    out, grad = np.empty(b, np.float64), np.empty((b, L, d), np.float32)
    rc = emu().sda_chain_log_prob_grad_host(ctypes.byref(model), U._p(x), b, L, L * d, d, U._p(out), U._p(grad))
    assert rc == 0, f'sda_chain_log_prob_grad_host rc={rc}'
    return out, grad


def emu_log_prob(chain, x):
    model = chain.model()
    x = np.ascontiguousarray(x, np.float32)
    b, L, d = x.shape
    out = np.empty(b, np.float64)
    assert U.emu().sda_chain_log_prob_host(ctypes.byref(model), U._p(x), b, L, L * d, d, U._p(out)) == 0
    return out


# ---------------------------------------------------------------- the oracle
_CACHE = {}


def oracles(key, fn, x):
    """(grad32, grad64) of the scalar fn(x) by torch autograd on the CPU, x taken in float32 and in float64; computed once per key."""
    if key not in _CACHE:
        out = []
        for dtype in (torch.float32, torch.float64):
            t = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_()
            out.append(torch.autograd.grad(fn(t), t)[0].numpy())
        _CACHE[key] = tuple(out)
    return _CACHE[key]


def advance_loss(chain, transitions, every, g):
    """x -> <chain.trajectory(x, transitions, last=not every), g> on the torch route (``chain`` is a default, grad='torch' chain)."""
    def fn(x):
        return (chain.trajectory(x, transitions, last=not every) * torch.from_numpy(g).to(x.dtype)).sum()
    return fn


def noisy_loss(chain, transitions, every, g, seed, row0, draw0):
    """The same for the noisy chain: the deterministic ``chain``'s rk4 with the row-keyed normals of philox_ref added as constants."""
    def fn(x):
        frames = []
        for t in range(transitions):
            z = philox_ref.randn_rows(x.shape[0], x.shape[1], seed, row0, draw0 + t)
            x = chain._rk4_transition(x) + torch.tensor(chain.dt ** 0.5, dtype=x.dtype) * torch.from_numpy(z).to(x.dtype)
            frames.append(x)
        out = torch.stack(frames) if every else x
        return (out * torch.from_numpy(g).to(x.dtype)).sum()
    return fn


def log_prior_loss(x):
    """The reference's log_prior recipe (experiments/lorenz/utils.py:82-88) on the torch route, summed over the trajectories."""
    chain = chains.NoisyLorenz63(dt=0.025)
    return chain.log_prob(x[..., :-1, :], x[..., 1:, :]).sum()


def noisy_trajectories(b, L, seed=3):
    """(b, L, 3) fp32: b trajectories of NoisyLorenz63(dt=0.025) from the fixture's states, by the host replay."""
    chain = chains.NoisyLorenz63(dt=0.025)
    x0 = U.golden()['l63/x0'][:b]
    frames = U.emu_advance(chain, x0, L - 1, True, seed=seed)
    return np.ascontiguousarray(np.concatenate((x0[None], frames)).transpose(1, 0, 2))


def check(case, got, ref32, ref64):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    b = U.bound(ref32, ref64)
    scale = float(np.abs(ref64).max())
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f'{case}: error {err:.3e} bound {b:.3e} scale {scale:.3e}')
    assert got.shape == ref64.shape, (case, got.shape, ref64.shape)
    assert b <= 1e-3 * scale, (case, 'the inputs leave a bound that cannot fail', b, scale)
    assert err <= b, (case, err, b)
