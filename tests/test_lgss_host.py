"""CPU: the linear-Gaussian state space of sda_amd/csrc/lgss.hip.  ``sda_lgss_tables`` (a host function, here through libsda_emu.so)
against dense Gaussian conditioning, the host replay of the four kernels' arithmetic against the same dense reference, the dense
probe, the rebinding of ``sda.mcs.DampedSpring`` and the ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains, ops
from tests import lgss_ref, philox_ref
from tests import lgss_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [('spring', 1, N) for N in (1, 2, 9)] + [('spring', 8, N) for N in (1, 2, 9)] + [('d8', 2, 4), ('d1', 3, 5)]


def _case(name, step):
    if name == 'spring':
        return U.spring_case(k=1, sigma=0.05, step=step)
    return U.random_case(8, 3, 7) if name == 'd8' else U.random_case(1, 1, 11)


@pytest.mark.parametrize('name,step,N', CASES)
def test_tables_against_dense_conditioning(name, step, N):
    """Both sides float64; the condition numbers of the default spring's covariances are below 1e6: 1e-9 of the largest entry."""
    case = _case(name, step)
    A, b, Q, m0, P0, H, c, sigma = case
    d, k, T = len(b), len(c), (N - 1) * step
    y = U.observations(case, step, N, 1, seed=N)[0]
    table = U.emu_tables(case, step, N)
    assert table.size == U.emu().sda_lgss_table_doubles(d, k, T)
    mean, cov, mf, logz = lgss_ref.tables_posterior(table, d, k, T, step, A, b, H, c, m0, y.astype(np.float64))
    want_mean, want_cov, want_logz = U.dense_posterior(case, step, y)
    assert np.abs(mean - want_mean).max() <= 1e-9 * np.abs(want_mean).max()
    assert np.abs(cov - want_cov).max() <= 1e-9 * np.abs(want_cov).max()
    assert abs(logz - want_logz) <= 1e-9 * max(abs(want_logz), 1.0)


def test_tables_refuse_a_q_that_is_not_positive_definite():
    case = list(U.spring_case())
    bad = case[2].copy()
    bad[3, 3] = -1.0
    case[2] = bad
    m = U.model64(tuple(case))
    table = np.empty(U.emu().sda_lgss_table_doubles(4, 1, 2))
    assert U.emu().sda_lgss_tables(ctypes.byref(m), 1, 3, U._p(table)) == -1
    semi = case[2].copy()
    semi[3, 3] = 0.0
    case[2] = semi
    assert U.emu().sda_lgss_tables(ctypes.byref(U.model64(tuple(case))), 1, 3, U._p(table)) == -1
    good = U.model64(U.spring_case())
    assert U.emu().sda_lgss_tables(ctypes.byref(good), 1, 3, U._p(table)) == 0
    assert U.emu().sda_lgss_tables(ctypes.byref(good), 0, 3, U._p(table)) == -1
    assert U.emu().sda_lgss_tables(None, 1, 3, U._p(table)) == -1
    assert U.emu().sda_lgss_table_doubles(9, 1, 2) == -1 and U.emu().sda_lgss_table_doubles(4, 0, 2) == -1
    assert U.emu().sda_lgss_table_doubles(4, 1, -1) == -1


def test_emulator_advance_is_the_keyed_affine_map():
    """Host replay of sda_lgss_advance: A = 0, b = 0, Lq = I returns the keyed normals themselves (to the 1e-6 by which the host's
    libm and numpy round log / sincos differently; on the device the comparison is bitwise); the spring follows the float64
    recursion on the same normals to 16 * 2^-24 (|b| + |A||x| + |Lq||z|) per transition."""
    seed, row0, draw0, m = 0x1234567890abcdef, 11, 5, 7
    ident = ops.lgss_model(torch.zeros(4, 4), torch.zeros(4), torch.eye(4))
    x = np.random.default_rng(0).standard_normal((m, 4)).astype(np.float32)
    out = np.empty((m, 4), np.float32)
    assert U.emu().sda_lgss_advance_host(ctypes.byref(ident), U._p(x), 4, m, 1, 0, U._p(out), 0, 4, seed, row0, draw0) == 0
    want = philox_ref.randn_rows(m, 4, seed, row0, draw0)
    assert np.abs(out - want).max() <= 1e-6 * np.abs(want).max()
    A, b, Q, _, _ = lgss_ref.spring()
    model = ops.lgss_model(torch.from_numpy(A), torch.from_numpy(b), torch.from_numpy(Q))
    Lq = np.array([[model.Lq[i][j] for j in range(4)] for i in range(4)], np.float64)
    traj = np.empty((5, m, 4), np.float32)
    assert U.emu().sda_lgss_advance_host(ctypes.byref(model), U._p(x), 4, m, 5, 1, U._p(traj), m * 4, 4, seed, row0, draw0) == 0
    ref, bound = x.astype(np.float64), np.zeros((m, 4))
    for t in range(5):
        z = philox_ref.randn_rows(m, 4, seed, row0, draw0 + t).astype(np.float64)
        bound = bound @ np.abs(A).T + 16 * 2.0 ** -24 * (np.abs(b) + np.abs(ref) @ np.abs(A).T + np.abs(z) @ np.abs(Lq).T)
        ref = ref @ A.T + b + z @ Lq.T
        assert (np.abs(traj[t] - ref) <= bound + 1e-6 * np.abs(z).max()).all()
    last = np.empty((m, 4), np.float32)
    assert U.emu().sda_lgss_advance_host(ctypes.byref(model), U._p(x), 4, m, 5, 0, U._p(last), 0, 4, seed, row0, draw0) == 0
    assert np.array_equal(last, traj[-1])


@pytest.mark.parametrize('name,step,N', [('spring', 8, 9), ('d8', 3, 2), ('d1', 1, 1)])
def test_emulator_filter_and_sampler(name, step, N):
    """Host replay of sda_lgss_filter against dense conditioning (1e-9) and of sda_lgss_sample against the float64 recursion on the
    same keyed normals (2^-22 of the largest value)."""
    case = _case(name, step)
    A, b, Q, m0, P0, H, c, sigma = case
    d, k, T, B, M = len(b), len(c), (N - 1) * step, 2, 5
    y = U.observations(case, step, N, B, seed=3)
    m64 = U.model64(case)
    table = U.emu_tables(case, step, N)
    mean = np.empty((B, T + 1, d))
    logz = np.empty(B)
    assert U.emu().sda_lgss_filter_host(ctypes.byref(m64), U._p(table), step, N, U._p(y), B, U._p(mean), U._p(logz)) == 0
    for s in range(B):
        _, _, mf, want_logz = lgss_ref.tables_posterior(table, d, k, T, step, A, b, H, c, m0, y[s].astype(np.float64))
        assert np.abs(mean[s] - mf).max() <= 1e-9 * np.abs(mf).max()
        assert abs(logz[s] - U.dense_posterior(case, step, y[s])[2]) <= 1e-9 * max(abs(want_logz), 1.0)
    out = np.empty((B, M, T + 1, d), np.float32)
    seed, draw0 = 99, 3
    assert U.emu().sda_lgss_sample_host(ctypes.byref(m64), U._p(table), U._p(mean), T, B, M, seed, 0, draw0, U._p(out)) == 0
    want = U.sample_ref(table, d, k, T, A, b, mean, M, lambda i: philox_ref.randn_rows(B * M, d, seed, 0, draw0 + i).astype(np.float64))
    assert np.abs(out - want).max() <= 2.0 ** -22 * np.abs(want).max()


@pytest.mark.parametrize('d,length', [(4, 1), (4, 2), (4, 9), (8, 5), (1, 4)])
@pytest.mark.parametrize('t', [1.0, 0.5, 0.0])
def test_emulator_exact_score(d, length, t):
    """Host replay of the block factor and the two sweeps against the dense float64 solve, and the symmetry the VJP relies on."""
    case = U.spring_case() if d == 4 else U.random_case(d, 1, d)
    A, b, Q, m0, P0 = case[:5]
    T = length - 1
    prec = ops.lgss_score_prec(*(torch.from_numpy(np.ascontiguousarray(v)) for v in (A, b, Q, m0, P0)), T).numpy()
    assert prec.size == U.emu().sda_lgss_score_doubles(d, T, 0)
    coef = np.array(lgss_ref.vp(t), np.float32)
    work = np.empty(U.emu().sda_lgss_score_doubles(d, T, 1))
    assert U.emu().sda_lgss_score_factor_host(d, T, U._p(prec), U._p(coef), U._p(work)) == 0
    n = 3
    rng = np.random.default_rng(length)
    x = rng.standard_normal((n, length, d)).astype(np.float32)
    Lam = lgss_ref.precision(A, Q, P0, T)
    m = lgss_ref.joint(A, b, Q, m0, P0, T)[0]
    for zero_mean in (0, 1):
        out = np.empty_like(x)
        ywork = np.empty(n * length * d)
        assert U.emu().sda_lgss_score_host(d, T, U._p(prec), U._p(coef), U._p(work), U._p(x), n, zero_mean, U._p(ywork), U._p(out)) == 0
        want = lgss_ref.eps_dense(x.astype(np.float64).reshape(n, -1), float(coef[0]), float(coef[1]), Lam, m * (1 - zero_mean))
        assert np.abs(out.reshape(n, -1) - want).max() <= 2.0 ** -22 * np.abs(want).max()


def test_probe_linear():
    chain = chains.DampedSpring()
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    H = torch.tensor([[1.0, -2.0, 0.5, 0.0], [0.0, 0.25, 0.0, 3.0]], dtype=torch.float64)
    c = torch.tensor([0.5, -1.0], dtype=torch.float64)
    got = chains.probe_linear(lambda x: x @ H.to(x).T + c.to(x), chain, 4)
    assert torch.allclose(got[0], H, atol=1e-14) and torch.allclose(got[1], c, atol=1e-14)
    sel = chains.probe_linear(lambda x: x[..., :1], chain, 4)
    assert torch.equal(sel[0], torch.eye(4, dtype=torch.float64)[:1]) and torch.equal(sel[1], torch.zeros(1, dtype=torch.float64))
    for bad in (lambda x: x ** 2, lambda x: x[..., :1].clamp(-0.5, 0.5), lambda x: x.sum()):
        assert chains.probe_linear(bad, chain, 4) is None
    assert torch.equal(torch.random.get_rng_state(), state)          # (the probe left the global generator alone)


def test_damped_spring_is_the_reference_chain_on_the_host_side():
    chain = chains.DampedSpring(dt=0.01)
    A, b, Q, m0, S0 = lgss_ref.spring()
    for got, want in ((chain.A, A), (chain.b, b), (chain.Sigma_x, Q), (chain.mu_0, m0), (chain.Sigma_0, S0)):
        assert torch.is_tensor(got) and got.dtype == torch.float32 and np.array_equal(got.numpy().astype(np.float64), want)
    assert chain.prior((5,)).shape == (5, 4)
    with pytest.raises(_lib.SdaHipError):
        chain.transition(torch.randn(5, 4))                          # no CPU fallback
    xg = torch.randn(5, 4, requires_grad=True)
    assert chain.transition(xg).shape == (5, 4)                      # ... but an input that requires grad takes the torch expression
    x1, x2 = torch.randn(3, 4), torch.randn(3, 4)
    want = torch.distributions.MultivariateNormal(x1 @ chain.A.T + chain.b, chain.Sigma_x).log_prob(x2)
    assert torch.equal(chain.log_prob(x1, x2), want)


def test_install_rebinds_damped_spring_in_subprocess():
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import sda_amd\n'
            'sda_amd.install_as_sda(native_chains=%s)\n'
            'import sda.mcs as M\n'
            'import sda_amd.chains as C\n'
            'try:\n'
            '    c = M.DampedSpring(dt=0.01)\n'
            '    print("CHAIN", M.DampedSpring is C.DampedSpring, tuple(c.A.shape))\n'
            'except ImportError as e:\n'
            '    print("PLACEHOLDER", M.DampedSpring is C.DampedSpring)\n')
    env = {k: v for k, v in os.environ.items() if k != 'SDA_MCS_FILE'}
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'True')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['CHAIN', 'True', '(4,', '4)']
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'False')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['PLACEHOLDER', 'False']


def test_abi_lists_the_lgss_entries(tmp_path):
    from sda_amd import build
    header = open(os.path.join(ROOT, 'include', 'sda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = sorted(set(re.findall(r'\b(sda_lgss_[a-z0-9_]+)\s*\(', text)))
    assert declared == sorted(['sda_lgss_advance', 'sda_lgss_table_doubles', 'sda_lgss_tables', 'sda_lgss_filter', 'sda_lgss_sample',
                               'sda_lgss_score_doubles', 'sda_lgss_score_factor', 'sda_lgss_score'])
    build.build()
    lib = _lib.load()
    for n in declared:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert '#define SDA_ABI_VERSION 14' in header and lib.sda_abi_version() == 14
    for mirror, ctype in (('LgssModel', 'sda_lgss_model'), ('LgssModel64', 'sda_lgss_model64')):
        Desc = getattr(_lib, mirror)
        fields = [f[0] for f in Desc._fields_]
        src = tmp_path / f'{mirror}.c'
        prints = '\n'.join(f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields)
        src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/sda_hip.h"\nint main(){{printf("size %zu\\n", '
                       f'sizeof({ctype}));\n{prints}\nreturn 0;}}')
        exe = tmp_path / mirror
        subprocess.check_call(['gcc', str(src), '-o', str(exe)])
        got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
        assert int(got['size']) == ctypes.sizeof(Desc)
        for f in fields:
            assert int(got[f]) == getattr(Desc, f).offset, (mirror, f)
    # bad arguments are refused on the host, before any launch
    assert lib.sda_lgss_advance(None, None, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, None) == -1
    assert lib.sda_lgss_filter(None, None, 1, 1, None, 1, None, None, None) == -1
    assert lib.sda_lgss_sample(None, None, None, 0, 1, 1, 0, 0, 0, None, None) == -1
    assert lib.sda_lgss_score_factor(0, 0, None, None, None, None) == -1
    assert lib.sda_lgss_score(4, -1, None, None, None, None, 1, 0, None, None, None) == -1
    good = U.model64(U.spring_case())
    assert lib.sda_lgss_filter(ctypes.byref(good), None, 1, 1, None, 1, None, None, None) == -1
    assert lib.sda_lgss_table_doubles(4, 1, 64) == 65 * (4 + 32 + 1 + 1)
