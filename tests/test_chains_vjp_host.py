"""CPU: the adjoint of the Markov chains (sda_chain_advance_vjp, sda_chain_log_prob_grad of sda_amd/csrc/chain.hip), replayed on
the host (libsda_emu.so runs the same __host__ __device__ functions as plain loops) against torch autograd through the torch-ops
``rk4`` in float64 (tests/chain_vjp_util.py: the oracle, the bound and what it requires of the inputs)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sda_amd import _lib, chains
from tests import chain_util as U
from tests import chain_vjp_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_UNSUPPORTED = -1, -2            # include/sda_hip.h


@pytest.mark.parametrize('every', [False, True])
@pytest.mark.parametrize('transitions', [1, 3])
@pytest.mark.parametrize('key', list(V.CHAINS))
def test_advance_vjp(key, transitions, every):
    """Every chain of the fixture and three sub-stepped ones (steps = 3: the recompute schedule), a random cotangent on every kept
    state.  The padded layout (particle stride d + 3 in every array) gives the same bits and leaves the gaps alone."""
    chain = V.make(key)
    x0 = V.x0_of(key)
    m, d = x0.shape
    g = V.cotangent((transitions, m, d) if every else (m, d), 11 * transitions + every)
    states = U.emu_advance(chain, x0, transitions, True)
    got = V.emu_vjp(chain, x0, states, g, transitions, every)
    r32, r64 = V.oracles(('adv', key, transitions, every), V.advance_loss(chain, transitions, every, g), x0)
    V.check(f'advance vjp {key} T={transitions} every={every}', got, r32, r64)
    assert np.array_equal(V.emu_vjp(chain, x0, states, g, transitions, every, pad=3), got)
    if transitions == 1:
        assert np.array_equal(V.emu_vjp(chain, x0, None, g, 1, every), got)        # one transition reads no stored state


@pytest.mark.parametrize('every', [False, True])
def test_noisy_advance_vjp(every):
    """Noise is additive: the stored states contain it and the Jacobian does not.  Oracle: float64 autograd of the deterministic
    rk4 with the same philox_ref normals added as constants."""
    chain = chains.NoisyLorenz63(dt=0.025)
    x0 = U.golden()['l63/x0']
    seed, row0, draw0, T = 0x1234567890abcdef, 11, 5, 5
    g = V.cotangent((T, 7, 3) if every else (7, 3), 21 + every)
    states = U.emu_advance(chain, x0, T, True, seed=seed, row0=row0, draw0=draw0)
    got = V.emu_vjp(chain, x0, states, g, T, every)
    det = chains.Lorenz63(dt=0.025)
    r32, r64 = V.oracles(('noisy', every), V.noisy_loss(det, T, every, g, seed, row0, draw0), x0)
    V.check(f'noisy advance vjp every={every}', got, r32, r64)
    # ... and it differs from the gradient along the noise-free trajectory: the states it reads are the noisy ones
    clean = V.emu_vjp(det, x0, U.emu_advance(det, x0, T, True), g, T, every)
    assert np.abs(clean - got).max() > 1e-3 * np.abs(got).max()


@pytest.mark.parametrize('b', [1, 5])
@pytest.mark.parametrize('L', [2, 3, 65, 130])
def test_log_prob_grad(L, b):
    """L = 2: one pair; 3: an interior index; 65: index 64 takes r_63 across the 64-index stride; 130: two hand-overs."""
    chain = chains.NoisyLorenz63(dt=0.025)
    x = V.noisy_trajectories(b, L)
    value, grad = V.emu_log_prob_grad(chain, x)
    assert np.array_equal(value, V.emu_log_prob(chain, x))
    r32, r64 = V.oracles(('lp', L, b), V.log_prior_loss, x)
    V.check(f'log_prob_grad L={L} b={b}', grad, r32, r64)


def test_log_prob_grad_lotka_volterra():
    """The other kind sda_chain_log_prob serves, with a noise level given to the model by hand (the class itself has none)."""
    chain = chains.LotkaVolterra(dt=0.05)
    x0 = U.golden()['lv/x0'][:3]
    frames = U.emu_advance(chain, x0, 8, True, noise=0.1, seed=9)
    x = np.ascontiguousarray(np.concatenate((x0[None], frames)).transpose(1, 0, 2))

    class Noisy(chains.LotkaVolterra):
        def _noise_std(self):
            return 0.1

    noisy = Noisy(dt=0.05)
    value, grad = V.emu_log_prob_grad(noisy, x)
    assert np.array_equal(value, V.emu_log_prob(noisy, x))

    def loss(t):
        mu = chains.LotkaVolterra(dt=0.05)._rk4_transition(t[:, :-1])
        return torch.distributions.Normal(mu, 0.1).log_prob(t[:, 1:]).sum()

    r32, r64 = V.oracles('lp_lv', loss, x)
    V.check('log_prob_grad lotka-volterra', grad, r32, r64)


def test_rows_do_not_depend_on_the_batch():
    for key in ('l63_s2', 'l96_5', 'l96_40', 'lv'):
        chain = V.make(key)
        x0 = V.x0_of(key)
        g = V.cotangent((3,) + x0.shape, 31)
        states = U.emu_advance(chain, x0, 3, True)
        full = V.emu_vjp(chain, x0, states, g, 3, True)
        one = V.emu_vjp(chain, x0[:1], np.ascontiguousarray(states[:, :1]), np.ascontiguousarray(g[:, :1]), 3, True)
        assert np.array_equal(one[0], full[0]), key
    chain = chains.NoisyLorenz63(dt=0.025)
    x = V.noisy_trajectories(5, 66)
    assert np.array_equal(V.emu_log_prob_grad(chain, x[:1])[1][0], V.emu_log_prob_grad(chain, x)[1][0])


def test_unsupported_and_bad_arguments():
    chain = V.make('l63')
    x0 = V.x0_of('l63')
    g = V.cotangent(x0.shape, 41)
    anc = np.arange(7, dtype=np.int32)
    assert V.emu_vjp(chain, x0, None, g, 1, False, anc=anc, rc_only=True) == E_UNSUPPORTED
    assert V.emu_vjp(chain, x0, None, g, 2, False, rc_only=True) == E_BADARG       # two transitions need the state between
    assert V.emu_vjp(chains.Lorenz96(n=65), np.zeros((1, 65), np.float32), None, np.zeros((1, 65), np.float32), 1, False,
                     rc_only=True) == E_UNSUPPORTED
    model = chains.Lorenz96(n=8).model()
    model.noise_std = 0.1
    x = np.zeros((1, 4, 8), np.float32)
    out, grad = np.empty(1), np.empty_like(x)
    rc = V.emu().sda_chain_log_prob_grad_host(ctypes.byref(model), U._p(x), 1, 4, 32, 8, U._p(out), U._p(grad))
    assert rc == E_UNSUPPORTED
    model = chains.NoisyLorenz63().model()
    assert V.emu().sda_chain_log_prob_grad_host(ctypes.byref(model), U._p(x), 1, 1, 3, 3, U._p(out), U._p(grad)) == E_BADARG


def test_abi_lists_the_adjoint_entries(tmp_path):
    from sda_amd import build
    header = open(os.path.join(ROOT, 'include', 'sda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    build.build()
    lib = _lib.load()
    for n in ('sda_chain_advance_vjp', 'sda_chain_log_prob_grad'):
        assert re.search(r'\b%s\s*\(' % n, text) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert '#define SDA_ABI_VERSION 14' in header and lib.sda_abi_version() == 14
    fields = [f[0] for f in _lib.ChainVjp._fields_]
    src = tmp_path / 'layout.c'
    prints = '\n'.join(f'printf("{f} %zu\\n", offsetof(sda_chain_vjp, {f}));' for f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/sda_hip.h"\nint main(){{printf("size %zu\\n", '
                   f'sizeof(sda_chain_vjp));\n{prints}\nreturn 0;}}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.ChainVjp)
    for f in fields:
        assert int(got[f]) == getattr(_lib.ChainVjp, f).offset, f
    # refused on the host, before any launch
    assert lib.sda_chain_advance_vjp(None, None) == E_BADARG
    assert lib.sda_chain_log_prob_grad(None, None, 0, 0, 0, 0, None, None, None) == E_BADARG


def test_python_routes_without_a_gpu():
    """What can be said of the Python layer on CPU tensors: they keep the torch route and record it, whatever ``grad`` says."""
    with pytest.raises(ValueError):
        chains.Lorenz63(grad='nonsense')
    for chain in (chains.Lorenz63(grad='device'), chains.Lorenz96(n=8, grad='device'), chains.NoisyLorenz63(dt=0.025, grad='device')):
        x = chain.prior((2,)).requires_grad_()
        chains.LAST_CHAIN_GRAD_ROUTE = None
        y = chain.trajectory(x, 2) if not isinstance(chain, chains.NoisyLorenz63) else chain.moments(x)[0]
        assert chains.LAST_CHAIN_GRAD_ROUTE == 'torch' and y.requires_grad
    with torch.no_grad():
        with pytest.raises(_lib.SdaHipError):
            chains.Lorenz63(grad='device').transition(torch.randn(2, 3).requires_grad_())
    assert chains.LAST_CHAIN_GRAD_ROUTE is None
