"""CPU: the Markov chains and the particle-filter arithmetic of sda_amd/csrc/chain.hip, replayed on the host (libsda_emu.so runs
the same __host__ __device__ functions as plain loops) against the reference's own outputs (tests/golden/chains.npz), and the
Python layer around them: the affine probe, the opt-in rebinding of sda.mcs, the ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains
from tests import chain_ref, philox_ref
from tests import chain_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23


@pytest.mark.parametrize('key', list(U.CHAINS))
def test_chain_ref_reproduces_reference_fp32(key):
    """chain_ref in fp32 against the reference's fp32 arrays.  Lorenz-63 and Lorenz-96 are +, -, x and / in a fixed order, each
    rounded once: bit-equal.  Lotka-Volterra calls exp, which libraries round differently: 2 ulp of the state scale."""
    g = U.golden()
    chain = U.make(key)
    x0 = g[f'{key}/x0']
    got1 = chain_ref.transition(*U.ref_args(chain), x0)
    gotn = chain_ref.trajectory(*U.ref_args(chain), x0, 16)
    assert got1.dtype == np.float32
    if key == 'lv':
        for got, ref in ((got1, g[f'{key}/trans32']), (gotn, g[f'{key}/traj32'])):
            assert np.abs(got - ref).max() <= 2 * ULP32 * np.abs(ref).max()
    else:
        assert np.array_equal(got1, g[f'{key}/trans32'])
        assert np.array_equal(gotn, g[f'{key}/traj32'])
    # and in float64 against the reference run on float64 inputs (exp again the only library call)
    got64 = chain_ref.trajectory(*U.ref_args(chain), x0.astype(np.float64), 16)
    assert np.abs(got64 - g[f'{key}/traj64']).max() <= 1e-14 * np.abs(g[f'{key}/traj64']).max()


def test_chain_ref_log_prob_and_processing():
    g = U.golden()
    chain = chains.NoisyLorenz63(dt=0.025)
    x = g['lp/x'].astype(np.float64)
    mu = chain_ref.transition(*U.ref_args(chain), x[:, :-1].reshape(-1, 3)).reshape(5, 8, 3)
    lp = chain_ref.normal_log_prob(x[:, 1:], mu, 0.025 ** 0.5).sum(-1)
    assert np.abs(lp - g['lp/log_prob64']).max() <= 1e-12 * np.abs(g['lp/log_prob64']).max()
    assert np.abs(lp.sum(-1) - g['lp/log_prior64']).max() <= 1e-12 * np.abs(g['lp/log_prior64']).max()
    ll = sum(chain_ref.logweights(x[:, 2 * i], [0], [0.0], [8.0], 0.25, g['lp/y'][:, i]) for i in range(5))
    assert np.abs(ll - g['lp/log_lik64']).max() <= 1e-12 * np.abs(g['lp/log_lik64']).max()
    xs = torch.from_numpy(g['pre/x'])
    assert np.array_equal(chains.Lorenz63.preprocess(xs).numpy(), g['pre/pre'])
    assert np.array_equal(chains.Lorenz63.postprocess(chains.Lorenz63.preprocess(xs)).numpy(), g['pre/post'])


@pytest.mark.parametrize('key', list(U.CHAINS))
def test_emulator_advance(key):
    """One transition and the 16-step trajectory of the kernel's arithmetic against the reference run in float64."""
    g = U.golden()
    chain = U.make(key)
    x0 = g[f'{key}/x0']
    got1 = U.emu_advance(chain, x0, 1, False)
    gotn = U.emu_advance(chain, x0, 16, True)
    last = U.emu_advance(chain, x0, 16, False)
    assert np.abs(got1 - g[f'{key}/trans64']).max() <= U.bound(g[f'{key}/trans32'], g[f'{key}/trans64'])
    assert np.abs(gotn - g[f'{key}/traj64']).max() <= U.bound(g[f'{key}/traj32'], g[f'{key}/traj64'])
    assert np.array_equal(last, gotn[-1]) and np.array_equal(got1, gotn[0])


def test_emulator_noisy_advance():
    """Noisy advance = deterministic advance + sqrt(dt) x the row-keyed normals of philox_ref, whatever row0 / draw0."""
    g = U.golden()
    chain = chains.NoisyLorenz63(dt=0.025)
    x0 = g['l63/x0']
    seed, row0, draw0 = 0x1234567890abcdef, 11, 5
    det = U.emu_advance(chain, x0, 1, False, noise=0.0)
    got = U.emu_advance(chain, x0, 1, False, seed=seed, row0=row0, draw0=draw0)
    want = det + np.float32(0.025 ** 0.5) * philox_ref.randn_rows(7, 3, seed, row0, draw0)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(got - det).max() > 1e-3
    # a 5-step noisy trajectory against chain_ref (noise re-enters the dynamics)
    traj = U.emu_advance(chain, x0, 5, True, seed=seed, row0=row0, draw0=draw0)
    ref = chain_ref.trajectory(*U.ref_args(chain), x0.astype(np.float64), 5, 0.025 ** 0.5, seed, row0, draw0)
    assert np.abs(traj - ref).max() <= U.bound(chain_ref.trajectory(*U.ref_args(chain), x0, 5, 0.025 ** 0.5, seed, row0, draw0), ref)


def test_emulator_log_prob_and_logweights():
    """Against the float64 fixture, to 1e-5 of the array's largest magnitude (a log-density is a sum of signed terms: where it
    crosses zero is arbitrary, so the error is measured against the array, not element by element)."""
    g = U.golden()
    chain = chains.NoisyLorenz63(dt=0.025)
    model = chain.model()
    x = np.ascontiguousarray(g['lp/x'], np.float32)
    out = np.empty(5, np.float64)
    rc = U.emu().sda_chain_log_prob_host(ctypes.byref(model), U._p(x), 5, 9, 27, 3, U._p(out))
    assert rc == 0
    assert np.abs(out - g['lp/log_prior64']).max() <= 1e-5 * np.abs(g['lp/log_prior64']).max()
    # strided: every trajectory as a pair (x_i, x_{i+1}) -> log_prob per pair
    pairs = np.empty(40, np.float64)
    for b in range(5):
        rc = U.emu().sda_chain_log_prob_host(ctypes.byref(model), U._p(x[b]), 8, 2, 3, 3, U._p(pairs[8 * b:]))
        assert rc == 0
    assert np.abs(pairs.reshape(5, 8) - g['lp/log_prob64']).max() <= 1e-5 * np.abs(g['lp/log_prob64']).max()
    # log-weights: log_likelihood of the fixture = the sum over the observed times of the per-state log-weights
    y = g['lp/y']
    ll = np.zeros(5)
    for i in range(5):
        for b in range(5):
            obs_b = U.emu_obs([0], [0.0], [8.0], 0.25, y[b, i])
            lw = np.empty(1, np.float32)
            xs = np.ascontiguousarray(x[b, 2 * i][None])
            assert U.emu().sda_bpf_logweights_host(U._p(xs), 1, 3, 3, ctypes.byref(obs_b), U._p(lw)) == 0
            ll[b] += lw[0]
    assert np.abs(ll - g['lp/log_lik64']).max() <= 1e-5 * np.abs(g['lp/log_lik64']).max()


@pytest.mark.parametrize('m,n,step', [(1, 1, 1), (65, 5, 3), (1000, 4, 2)])
def test_emulator_ancestors_and_traceback(m, n, step):
    """The ancestor search and the traceback index walk, bit-equal to chain_ref's searchsorted and literal cat / re-gather."""
    rng = np.random.default_rng(m)
    S = rng.standard_normal((n * step + 1, m, 3)).astype(np.float32)
    anc = np.empty((n, m), np.int32)
    for k in range(n):
        w = rng.random(m).astype(np.float32) ** 4
        ref, cdf, _, margin = chain_ref.ancestors(w, 77, k, return_margin=True)
        assert margin.min() > 1e-12                  # (no draw sits on a boundary: the comparison below is unambiguous)
        assert U.emu().sda_bpf_resample_host(U._p(cdf), m, 77, k, U._p(anc[k])) == 0
        assert np.array_equal(anc[k], ref)
    out = np.empty((m, n * step + 1, 3), np.float32)
    assert U.emu().sda_bpf_traceback_host(U._p(S), m * 3, 3, U._p(anc), m, n, step, 3, U._p(out)) == 0
    assert np.array_equal(out, chain_ref.regather(S, anc, step))


def test_affine_probe():
    chain = chains.NoisyLorenz63(dt=0.025)
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    a = chains.probe_affine(lambda x: chains.Lorenz63.preprocess(x)[..., :1], chain, 3)
    assert (a.index, a.shift, a.scale) == ([0], [0.0], [8.0])
    b = chains.probe_affine(lambda x: x[..., ::2], chain, 3)
    assert (b.index, b.shift, b.scale) == ([0, 2], [0.0, 0.0], [1.0, 1.0])
    c = chains.probe_affine(lambda x: chains.Lorenz63.preprocess(x)[..., 2:], chain, 3)
    assert c.index == [2] and abs(c.shift[0] - 25.0) < 1e-12 and abs(c.scale[0] - 8.6) < 1e-12
    x = chain.prior((9,))
    assert torch.equal(c(x), chains.Lorenz63.preprocess(x)[..., 2:])
    for bad in (lambda x: x[..., :1] ** 2, lambda x: x.sum(-1, keepdim=True), lambda x: x[..., :1].clamp(-3, 3),
                lambda x: x.clamp(-1, 1)):
        assert chains.probe_affine(bad, chain, 3) is None
    torch.set_rng_state(state)
    assert torch.equal(torch.random.get_rng_state(), state)          # (the probe left the global generator alone)
    assert chains.probe_affine(a, chain, 3) is a


def test_user_subclass_falls_back_to_torch_rk4():
    class Mine(chains.DiscreteODE):
        def prior(self, shape=(), *, device=None):
            return torch.randn(*shape, 2)

        def f(self, x):
            return -x

    class Tweaked(chains.Lorenz63):
        def f(self, x):
            return super().f(x) * 0.5

    x = torch.randn(4, 2)
    got = Mine(dt=0.1, steps=2).trajectory(x, 3)                    # CPU tensors: only the torch route can serve them
    assert got.shape == (3, 4, 2)
    assert torch.allclose(got[-1], x * np.exp(-0.3), rtol=1e-4)
    assert Tweaked().transition(torch.randn(5, 3)).shape == (5, 3)
    with pytest.raises(_lib.SdaHipError):
        chains.Lorenz63().transition(torch.randn(5, 3))              # the built-in system has no CPU fallback
    xg = torch.randn(5, 3, requires_grad=True)
    chains.Lorenz63().transition(xg).sum().backward()               # ... but autograd gets the torch-ops rk4
    assert xg.grad is not None


def test_install_native_chains_in_subprocess():
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import sda_amd\n'
            'sda_amd.install_as_sda(native_chains=%s)\n'
            'from sda.mcs import *\n'
            'import sda.mcs as M\n'
            'try:\n'
            '    c = NoisyLorenz63(dt=0.025)\n'
            '    print("CHAIN", type(c).__module__, M.SOURCE, c.dt)\n'
            'except ImportError as e:\n'
            '    print("PLACEHOLDER", M.SOURCE)\n')
    env = {k: v for k, v in os.environ.items() if k != 'SDA_MCS_FILE'}
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'True')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ['CHAIN', 'sda_amd.chains', 'sda_amd.chains', '0.025']
    out = subprocess.run([sys.executable, '-B', '-c', code % (ROOT, 'False')], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[0] == 'PLACEHOLDER'


def test_abi_lists_the_chain_entries(tmp_path):
    from sda_amd import build
    header = open(os.path.join(ROOT, 'include', 'sda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = ['sda_chain_advance', 'sda_chain_log_prob', 'sda_bpf_logweights', 'sda_bpf_logweights_blocks', 'sda_bpf_cdf',
             'sda_bpf_resample', 'sda_bpf_traceback']
    build.build()
    lib = _lib.load()
    for n in names:
        assert re.search(r'\b%s\s*\(' % n, text) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert '#define SDA_ABI_VERSION 14' in header and lib.sda_abi_version() == 14
    # the ctypes mirrors of the three new structs against what gcc sees
    for mirror, ctype in (('ChainModel', 'sda_chain_model'), ('ChainObs', 'sda_chain_obs'), ('ChainAdv', 'sda_chain_adv')):
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
    assert lib.sda_chain_advance(None, None) == -1
    assert lib.sda_bpf_cdf(None, 0, None, 0, None, None, None, None) == -1
    assert lib.sda_bpf_logweights_blocks(5000) == 20
