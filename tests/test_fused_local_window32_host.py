"""CPU: the argument checks of the fused local route's launches (sda_mlp_fwd_win, sda_mlp_bwd_win, sda_mc_finish) at the window limit of 32
values -- every call here returns before anything is launched -- and the ABI version, which the two-fragment windows did not move."""
import ctypes

import pytest

BADARG, UNSUPPORTED = -1, -2
PTR = 1 << 20               # a non-null, 16-byte aligned address that is never dereferenced


@pytest.fixture(scope='module')
def lib():
    from sda_amd import _lib
    return _lib.load()


def _desc(wc, emb_n=32):
    from sda_amd import _lib
    d = _lib.MlpDesc()
    d.rows, d.ngemm = 4, 1
    d.kind[0], d.in_f[0], d.out_f[0] = 0, wc + emb_n, wc
    d.w, d.bias = PTR, PTR
    return d


def _win(k, c, nw=4, emb_n=32):
    from sda_amd import _lib
    w = _lib.MlpWin()
    w.nw, w.len, w.c, w.emb_n = nw, nw + 2 * k, c, emb_n
    w.x = w.emb = w.coef = w.y = w.eps = w.ghat = PTR
    w.cn = 1.0
    w.p_start, w.p_step, w.p_stop = 0, 1, nw + 2 * k
    w.c_start, w.c_step, w.c_stop = 0, 1, c
    return w


@pytest.mark.parametrize('k,c', [(5, 3), (1, 11)])
def test_windows_of_33_values_are_unsupported(lib, k, c):
    assert (2 * k + 1) * c == 33
    d, w = _desc(33), _win(k, c)
    w.gwin = PTR
    assert lib.sda_mlp_fwd_win(ctypes.byref(d), ctypes.byref(w), None) == UNSUPPORTED
    assert lib.sda_mlp_bwd_win(ctypes.byref(d), ctypes.byref(w), None) == UNSUPPORTED


@pytest.mark.parametrize('k,c', [(4, 3), (3, 3), (2, 6), (0, 32)])
def test_windows_up_to_32_values_pass_the_limit_and_keep_the_gwin_checks(lib, k, c):
    """A window of 17 .. 32 values gets past the limit: what rejects these calls is the check behind it (a null, then a misaligned gwin)."""
    d, w = _desc((2 * k + 1) * c), _win(k, c)
    assert lib.sda_mlp_bwd_win(ctypes.byref(d), ctypes.byref(w), None) == BADARG
    w.gwin = PTR + 4
    assert lib.sda_mlp_bwd_win(ctypes.byref(d), ctypes.byref(w), None) == BADARG


@pytest.mark.parametrize('k,c', [(5, 3), (1, 11), (16, 1)])
def test_mc_finish_rejects_windows_of_33_values(lib, k, c):
    assert (2 * k + 1) * c == 33
    assert lib.sda_mc_finish(PTR, PTR, PTR, 2, 4, k, c, 0.0, 0.0, PTR, 0, PTR, None, None, None, None) == BADARG


def test_abi_version_is_unchanged(lib):
    assert lib.sda_abi_version() == 14
