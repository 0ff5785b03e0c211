"""TEST-ONLY helpers shared by tests/test_chains_host.py and tests/test_gpu_chains.py: the chains.npz fixture, the chains it was
generated for, the error bound of the transition tests and the ctypes binding of the host replay (libsda_emu.so)."""
import ctypes
import functools
import os

import numpy as np

from sda_amd import _lib, chains

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chains.npz')

#: fixture name -> (class name, constructor arguments): tests/golden/make_golden_chains.py CHAINS
CHAINS = {
    'l63': ('Lorenz63', {}),
    'l63_s2': ('Lorenz63', {'dt': 0.025, 'steps': 2}),
    'l96_4': ('Lorenz96', {'n': 4}),
    'l96_5': ('Lorenz96', {'n': 5}),
    'l96_32': ('Lorenz96', {'n': 32}),
    'l96_40': ('Lorenz96', {'n': 40}),
    'l96_64': ('Lorenz96', {'n': 64}),
    'lv': ('LotkaVolterra', {}),
}
KIND_NAMES = {0: 'lorenz63', 1: 'lotka_volterra', 2: 'lorenz96'}


@functools.lru_cache(None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def make(key):
    cls, kw = CHAINS[key]
    return getattr(chains, cls)(**kw)


def ref_args(chain):
    """(kind, params, dt, steps) for tests/chain_ref.py."""
    model = chain.model()
    d, params = chain._params()
    return KIND_NAMES[model.kind], params, chain.dt, chain.steps


def bound(ref32, ref64):
    """The repository's '3 x own error' rule: max(1e-6 max|x|, 3 x |reference fp32 - reference fp64|), one number per array."""
    return max(1e-6 * np.abs(ref64).max(), 3 * np.abs(ref32.astype(np.float64) - ref64).max())


@functools.lru_cache(None)
def emu():
    from sda_amd import build
    lib = ctypes.CDLL(build.build_emu())
    P = ctypes.c_void_p
    sig = {
        'sda_chain_advance_host': [ctypes.POINTER(_lib.ChainAdv)],
        'sda_chain_log_prob_host': [ctypes.POINTER(_lib.ChainModel), P, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, P],
        'sda_bpf_logweights_host': [P, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(_lib.ChainObs), P],
        'sda_bpf_resample_host': [P, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, P],
        'sda_bpf_traceback_host': [P, ctypes.c_int64, ctypes.c_int64, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, args
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_advance(chain, x, length, every, *, noise=None, seed=0, row0=0, draw0=0, anc=None):
    """Host replay of sda_chain_advance on a numpy (m, d) fp32 array -> (length, m, d) or (m, d)."""
    model = chain.model()
    if noise is not None:
        model.noise_std = noise
    x = np.ascontiguousarray(x, np.float32)
    m, d = x.shape
    out = np.empty((length, m, d) if every else (m, d), np.float32)
    a = _lib.ChainAdv()
    a.model = model
    a.x_in, a.in_sp = x.ctypes.data, d
    a.anc = None if anc is None else anc.ctypes.data
    a.out, a.out_st, a.out_sp, a.every = out.ctypes.data, m * d, d, int(every)
    a.m, a.transitions, a.seed, a.row0, a.draw0 = m, length, seed, row0, draw0
    rc = emu().sda_chain_advance_host(ctypes.byref(a))
    assert rc == 0, f'sda_chain_advance_host rc={rc}'
    return out


def emu_obs(index, shift, scale, sigma, y):
    o = _lib.ChainObs()
    o.k = len(index)
    for i in range(o.k):
        o.idx[i], o.shift[i], o.scale[i] = index[i], shift[i], scale[i]
    o.sigma = sigma
    y = np.ascontiguousarray(y, np.float32)
    o.y = y.ctypes.data
    o._keep = y
    return o
