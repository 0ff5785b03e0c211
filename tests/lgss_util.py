"""Shared by the linear-Gaussian tests: the host replay of csrc/lgss.hip (libsda_emu.so) behind numpy wrappers, and the models."""
import ctypes
import functools

import numpy as np
import torch

from sda_amd import _lib, ops
from tests import lgss_ref

P = ctypes.c_void_p
I, I64, U64 = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64


@functools.lru_cache(maxsize=None)
def emu():
    from sda_amd import build
    lib = ctypes.CDLL(build.build_emu())
    M, M64 = ctypes.POINTER(_lib.LgssModel), ctypes.POINTER(_lib.LgssModel64)
    sig = {
        'sda_lgss_advance_host': (I, [M, P, I64, I, I, I, P, I64, I64, U64, I64, I64]),
        'sda_lgss_table_doubles': (I64, [I, I, I]),
        'sda_lgss_tables': (I, [M64, I, I, P]),
        'sda_lgss_filter_host': (I, [M64, P, I, I, P, I, P, P]),
        'sda_lgss_sample_host': (I, [M64, P, P, I, I, I, U64, I64, I64, P]),
        'sda_lgss_score_doubles': (I64, [I, I, I]),
        'sda_lgss_score_factor_host': (I, [I, I, P, P, P]),
        'sda_lgss_score_host': (I, [I, I, P, P, P, P, I, I, P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _p(a):
    return a.ctypes.data_as(P)


def spring_case(k=1, sigma=0.05, burn=64, step=1):
    """(A, b, Q, m0, P0, H, c, sigma): the default spring observed through its first k components, at the first returned state."""
    A, b, Q, m0, S0 = lgss_ref.spring()
    m, Pm = lgss_ref.push(A, b, Q, m0, S0, burn + step)
    return A, b, Q, m, Pm, np.eye(4)[:k], np.zeros(k), sigma


def random_case(d, k, seed, sigma=0.3):
    A, b, Q, m0, S0, H, c = lgss_ref.random_model(d, k, seed)
    return A, b, Q, m0, S0, H, c, sigma


def model64(case):
    return ops.lgss_model64(*(torch.from_numpy(np.ascontiguousarray(v)) for v in case[:7]), case[7])


def emu_tables(case, step, N):
    return ops.lgss_tables(model64(case), step, N, lib=emu()).numpy()


def observations(case, step, N, B, seed):
    """B sequences of N observations drawn from the model itself (float64), rounded to fp32 as the kernels read them."""
    A, b, Q, m0, P0, H, c, sigma = case
    rng = np.random.default_rng(seed)
    d, T = len(b), (N - 1) * step
    Lq, L0 = np.linalg.cholesky(Q), np.linalg.cholesky(P0)
    y = np.empty((B, N, len(c)))
    for s in range(B):
        x = m0 + L0 @ rng.standard_normal(d)
        for i in range(T + 1):
            if i:
                x = A @ x + b + Lq @ rng.standard_normal(d)
            if i % step == 0:
                y[s, i // step] = H @ x + c + sigma * rng.standard_normal(len(c))
    return y.astype(np.float32)


def dense_posterior(case, step, y):
    """Dense conditioning on one sequence y (N, k): posterior mean ((T + 1) d,), covariance, log p(y)."""
    A, b, Q, m0, P0, H, c, sigma = case
    T = (len(y) - 1) * step
    mean, cov = lgss_ref.joint(A, b, Q, m0, P0, T)
    Hb, cb = lgss_ref.observe(H, c, T, step, len(b))
    return lgss_ref.condition(mean, cov, Hb, cb, sigma, y.astype(np.float64).reshape(-1))


def sample_ref(table, d, k, T, A, b, mean, M, z):
    """The two recursions of sda_lgss_sample in float64 numpy; z(i): the (B M, d) normals of time i."""
    B = mean.shape[0]
    tab = table.reshape(T + 1, -1)
    G = tab[:, d * k:d * k + d * d].reshape(T + 1, d, d)
    L = tab[:, d * k + d * d:d * k + 2 * d * d].reshape(T + 1, d, d)
    want = np.empty((B, M, T + 1, d))
    for i in range(T, -1, -1):
        zi = z(i).reshape(B, M, d)
        mi = mean[:, None, i]
        if i == T:
            want[:, :, i] = mi + zi @ L[i].T
        else:
            want[:, :, i] = mi + (want[:, :, i + 1] - (mi @ A.T + b)) @ G[i].T + zi @ L[i].T
    return want
