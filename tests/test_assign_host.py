"""CPU: the epsilon-scaling auction of sda_amd/csrc/assign.hip, replayed on the host (libsda_emu.so runs the kernel's
__host__ __device__ bid, resolve and certificate functions with lanes and waves as loops), against
scipy.optimize.linear_sum_assignment and the project's own exact host solver (ops.assignment_cost)."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from sda_amd import ops
from tests import assign_util as A


def exact_cols(cost):
    rows, cols = linear_sum_assignment(cost.astype(np.float64))
    assert (rows == np.arange(len(rows))).all()
    return cols


def solve(name, **kw):
    cost = A.cases()[name]
    rc, res = A.host_auction(cost, **kw)
    assert rc == 0
    return cost, res


@pytest.mark.parametrize('n', A.RANDOM_NS)
def test_random_euclidean_costs(n):
    cost, res = solve(f'euclid{n}')
    exact = A.check_certificate(cost, res, exact_cols(cost))
    total, cols = ops.assignment_cost(torch.from_numpy(cost.copy()))            # the project's exact host solver agrees
    assert abs(total - exact) <= 1e-12 * max(abs(exact), 1.0)
    assert int(res['bids']) <= A.default_budget(n)
    if n == 1:
        assert int(res['bids']) == 0 and float(res['gap']) == 0.0


def test_integer_costs_are_solved_exactly():
    """Integer costs in [0, 100]: with n eps_final < 1 the certificate leaves no room for a suboptimal integer total."""
    cost = A.cases()['integer40']
    n = cost.shape[0]
    eps_rel = 1.0 / (2 * n * 100)
    R = float(cost.max()) - float(cost.min())
    assert n * (eps_rel * R) < 1                                                 # checked on the inputs, before the solve
    rc, res = A.host_auction(cost, eps_rel=eps_rel)
    assert rc == 0 and float(res['eps_final']) == eps_rel * R and n * float(res['eps_final']) < 1
    exact = A.check_certificate(cost, res, exact_cols(cost))
    assert float(res['total']) == exact and float(res['total']) == round(exact)


def test_all_equal_costs_give_the_identity_without_bids():
    cost, res = solve('all_equal')
    n = cost.shape[0]
    assert int(res['status']) == A.OK and int(res['bids']) == 0
    assert (res['col_of_row'] == np.arange(n)).all()
    assert float(res['gap']) == 0.0 and float(res['eps_final']) == 0.0 and float(res['total']) == 2.5 * n


def test_x_equal_y_costs_nothing():
    cost, res = solve('x_eq_y')
    A.check_certificate(cost, res, np.arange(cost.shape[0]))
    assert float(res['total']) == 0.0 and (res['col_of_row'] == np.arange(cost.shape[0])).all()


@pytest.mark.parametrize('name', ['duplicates', 'i_times_j', 'far_column'])
def test_degenerate_costs(name):
    cost, res = solve(name)
    A.check_certificate(cost, res, exact_cols(cost))
    assert int(res['bids']) <= A.default_budget(cost.shape[0])


def test_runs_are_repeatable_bit_for_bit():
    cost = A.cases()['duplicates']
    _, a = A.host_auction(cost)
    _, b = A.host_auction(cost.copy())
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_costs_are_rejected(bad):
    cost = A.cases()['euclid5'].copy()
    cost[3, 1] = bad
    rc, res = A.host_auction(cost, guard=8)
    assert rc == 0 and int(res['status']) == A.BADARG and int(res['bids']) == 0
    both = np.stack([A.cases()['euclid5'], cost])                                # ... and only the problem that holds it
    rc, res = A.host_auction(both)
    assert rc == 0 and res['status'].tolist() == [A.OK, A.BADARG]


def test_sizes_and_arguments_outside_the_range():
    big = np.zeros((4097, 4097), np.float32)
    rc, _ = A.host_auction(big, guard=8)
    assert rc == A.UNSUPPORTED                                                   # not served
    assert ops.AUCTION_MAX_N == 4096
    c = A.cases()['euclid5']
    assert A.host_auction(c, eps_rel=0.0)[0] == A.BADARG
    assert A.host_auction(c, eps_rel=float('nan'))[0] == A.BADARG
    assert A.host_auction(c, bid_budget=0)[0] == A.BADARG
    fn = A.emu().sda_assignment_auction_host
    assert fn(None, 5, 1, 1e-7, 10, None, None, None, None, None, None) == A.BADARG


def test_tiny_budget_stops_early_and_writes_nothing_else():
    cost = A.cases()['euclid64']
    rc, res = A.host_auction(cost, bid_budget=1, guard=16)                       # (the guard bands are checked inside)
    assert rc == 0 and int(res['status']) == A.NOT_CONVERGED and int(res['bids']) <= 1
    assert np.isnan(res['total']) and np.isnan(res['gap']) and float(res['eps_final']) > 0
    assert ((res['col_of_row'] >= -1) & (res['col_of_row'] < 64)).all()
    # a budget that ends inside the first phase: the partial state is a partial matching
    rc, res = A.host_auction(cost, bid_budget=100, guard=16)
    assert int(res['status']) == A.NOT_CONVERGED and 64 <= int(res['bids']) <= 100
    taken = res['col_of_row'][res['col_of_row'] >= 0]
    assert len(set(taken.tolist())) == len(taken)
    # and the smallest budget that suffices gives the default run's answer
    _, full = A.host_auction(cost)
    rc, res = A.host_auction(cost, bid_budget=int(full['bids']), guard=16)
    assert int(res['status']) == A.OK and all(np.array_equal(res[k], full[k]) for k in full)
    assert int(A.host_auction(cost, bid_budget=int(full['bids']) - 1)[1]['status']) == A.NOT_CONVERGED


def test_batch_equals_single_calls():
    rng = np.random.default_rng(7)
    batch = np.stack([A.euclid(rng, 24, scale=1.0 + k) for k in range(8)])
    batch[5] = np.round(batch[5] * 4)                                            # one with ties
    rc, res = A.host_auction(batch, guard=8)
    assert rc == 0
    for k in range(8):
        _, one = A.host_auction(batch[k])
        for key in one:
            assert np.array_equal(res[key][k], one[key]), (k, key)


def test_python_layer_refuses_host_tensors_and_odd_shapes():
    from sda_amd._lib import SdaHipError
    with pytest.raises(SdaHipError):
        ops.assignment_auction(torch.zeros(4, 4))                                # a CPU tensor: no CPU path
    from sda_amd import metrics
    assert metrics.EMD_SOLVER == 'host' and metrics.LAST_EMD_ROUTE in (None, 'host', 'device', 'host_fallback')
    with pytest.raises(ValueError):
        metrics.emd(torch.zeros(3, 2), torch.zeros(3, 2), solver='simplex')
