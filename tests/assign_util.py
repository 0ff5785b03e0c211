"""Shared by tests/test_assign_host.py and tests/test_gpu_assign.py: the ctypes binding of the auction's host replay
(sda_assignment_auction_host in libsda_emu.so), the list of cost matrices both files run, and the checks every converged
result must pass."""
import ctypes
import functools
import math

import numpy as np

OK, NOT_CONVERGED, BADARG, UNSUPPORTED = 0, 1, -1, -2
WAVES = 16                      # AU_WAVES of csrc/assign.hip: wave w adds rows w, w + 16, ... of the certificate sums


@functools.lru_cache(maxsize=None)
def emu():
    from sda_amd import build
    lib = ctypes.CDLL(build.build_emu())
    P = ctypes.c_void_p
    fn = lib.sda_assignment_auction_host
    fn.restype = ctypes.c_int
    fn.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int64, P, P, P, P, P, P]
    return lib


def default_budget(n):
    from sda_amd import ops
    return ops.auction_default_budget(n)


def host_auction(cost, eps_rel=1e-7, bid_budget=None, guard=0):
    """Host replay on a numpy (n, n) or (b, n, n) fp32 array -> (rc, dict of per-problem arrays).  guard > 0 places that many
    sentinel elements before and after every output array and asserts that they are intact afterwards."""
    cost = np.ascontiguousarray(cost, np.float32)
    single = cost.ndim == 2
    n = cost.shape[-1]
    b = 1 if single else cost.shape[0]
    if bid_budget is None:
        bid_budget = default_budget(n)
    spec = {'total': (np.float64, b), 'gap': (np.float64, b), 'eps_final': (np.float64, b), 'bids': (np.int64, b),
            'status': (np.int32, b), 'col_of_row': (np.int32, b * n)}
    SENT = 0x5A
    bufs = {k: np.full((count + 2 * guard) * np.dtype(dt).itemsize, SENT, np.uint8) for k, (dt, count) in spec.items()}
    view = {k: bufs[k].view(dt)[guard:guard + count] for k, (dt, count) in spec.items()}
    rc = emu().sda_assignment_auction_host(cost.ctypes.data, n, b, eps_rel, bid_budget, *(view[k].ctypes.data for k in spec))
    for k, (dt, count) in spec.items():
        size = np.dtype(dt).itemsize
        assert (bufs[k][:guard * size] == SENT).all() and (bufs[k][(guard + count) * size:] == SENT).all(), f'{k}: guard band overwritten'
    out = {k: v.copy() for k, v in view.items()}
    out['col_of_row'] = out['col_of_row'].reshape(b, n)
    if single:
        out = {k: v[0] for k, v in out.items()}
    return rc, out


def euclid(rng, n, d=3, scale=1.0):
    x, y = rng.standard_normal((n, d)) * scale, rng.standard_normal((n, d)) * scale
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)).astype(np.float32)


RANDOM_NS = (1, 2, 3, 5, 63, 64, 65, 127, 257)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> fp32 cost matrix: the list both the host-replay tests and the device parity test run (left unchanged by them)."""
    rng = np.random.default_rng(20240611)
    out = {}
    for n in RANDOM_NS:
        out[f'euclid{n}'] = euclid(rng, n)
    out['integer40'] = rng.integers(0, 101, (40, 40)).astype(np.float32)
    out['all_equal'] = np.full((37, 37), 2.5, np.float32)
    x = rng.standard_normal((48, 3))
    out['x_eq_y'] = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1)).astype(np.float32)
    xd, yd = np.repeat(rng.standard_normal((6, 3)), 8, 0), np.repeat(rng.standard_normal((4, 3)), 12, 0)
    out['duplicates'] = np.sqrt(((xd[:, None] - yd[None]) ** 2).sum(-1)).astype(np.float32)            # many exact ties
    i = np.arange(33, dtype=np.float64)
    out['i_times_j'] = np.outer(i, i).astype(np.float32)
    far = euclid(rng, 50)
    far[:, 17] += 1e4                                                                                    # one column far dearer
    out['far_column'] = far
    for v in out.values():
        v.setflags(write=False)
    return out


def selected_sum(cost, cols):
    """sum_i cost[i][cols[i]] in float64 in the kernel's order: per wave over its rows in row order, then the waves in order."""
    n = cost.shape[0]
    total = 0.0
    for w in range(WAVES):
        part = 0.0
        for i in range(w, n, WAVES):
            part += float(cost[i, cols[i]])
        total += part
    return total


def check_certificate(cost, res, exact_cols):
    """The properties of a converged solve: a permutation, total is the selected sum, 0 <= total - exact <= gap (+ round-off),
    gap <= n eps_final.  `exact_cols`: an optimal permutation from an exact solver.  The lower bound compares the two selections'
    correctly rounded sums (math.fsum), so that it is not at the mercy of the order in which either solver adds its costs."""
    n = cost.shape[0]
    cols = np.asarray(res['col_of_row'])
    total, gap, eps_final = float(res['total']), float(res['gap']), float(res['eps_final'])
    assert int(res['status']) == OK
    assert sorted(cols.tolist()) == list(range(n)), 'col_of_row is not a permutation'
    assert total == selected_sum(cost, cols)
    mine = math.fsum(float(cost[i, cols[i]]) for i in range(n))
    exact_total = math.fsum(float(cost[i, exact_cols[i]]) for i in range(n))
    assert abs(total - mine) <= 1e-12 * abs(total)
    print(f'n={n} total={total!r} exact={exact_total!r} gap={gap:.3e} n*eps_final={n * eps_final:.3e} bids/n={int(res["bids"]) / n:.1f}')
    assert 0 <= mine - exact_total
    assert total - exact_total <= gap + 1e-9 * abs(total)
    assert gap <= n * eps_final * (1 + 1e-9)
    return exact_total
