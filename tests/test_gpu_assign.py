"""GPU: the auction kernel of sda_amd/csrc/assign.hip against its host replay (bit for bit), against the exact host solver
(certificate inequalities), and the routes of metrics.emd around it."""
import numpy as np
import pytest
import torch

from tests import assign_util as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def device_auction(cost, dev, **kw):
    from sda_amd import ops
    res = ops.assignment_auction(cost if torch.is_tensor(cost) else torch.from_numpy(np.array(cost, np.float32)).to(dev), **kw)
    return {k: getattr(res, k).cpu().numpy() for k in ('total', 'gap', 'eps_final', 'bids', 'status', 'col_of_row')}


def assert_same(got, ref, what):
    """Device result == host replay, every output bit for bit (NaN == NaN: the not-converged and rejected records).  The
    certificate sums are replayed in the kernel's own order (per-wave partial sums in row order, the shuffle tree of the price
    sum, the wave totals in order), so total and gap need no tolerance."""
    for k in ('col_of_row', 'status', 'bids'):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    for k in ('total', 'gap', 'eps_final'):
        assert np.array_equal(np.asarray(got[k]).view(np.int64), np.asarray(ref[k]).view(np.int64)), (what, k, got[k], ref[k])


def test_parity_with_host_replay(dev):
    for name, cost in A.cases().items():
        rc, ref = A.host_auction(cost)
        assert rc == 0
        assert_same(device_auction(cost, dev), ref, name)
    c64 = A.cases()['euclid64']
    for budget in (1, 100):                                                      # budget exhausted: the same partial state
        _, ref = A.host_auction(c64, bid_budget=budget)
        got = device_auction(c64, dev, bid_budget=budget)
        assert int(got['status']) == A.NOT_CONVERGED and int(got['bids']) <= budget
        assert_same(got, ref, f'budget{budget}')
    _, ref = A.host_auction(A.cases()['integer40'], eps_rel=1.0 / 8000)
    assert_same(device_auction(A.cases()['integer40'], dev, eps_rel=1.0 / 8000), ref, 'integer40 exact')
    bad = A.cases()['euclid5'].copy()
    bad[2, 2] = np.nan
    _, ref = A.host_auction(bad)
    got = device_auction(bad, dev)
    assert int(got['status']) == A.BADARG
    assert_same(got, ref, 'nan')


def test_batch_on_device_equals_host_replay_and_guards_hold(dev):
    from sda_amd import ops
    rng = np.random.default_rng(7)
    batch = np.stack([A.euclid(rng, 24, scale=1.0 + k) for k in range(8)])
    batch[5] = np.round(batch[5] * 4)
    batch[6, 3, 3] = np.inf                                                      # one rejected problem among the eight
    _, ref = A.host_auction(batch)
    assert_same(device_auction(batch, dev), ref, 'batch')
    # the C entry on caller-owned buffers with guard bands around every output
    lib = ops._lib.load()
    g, n, b = 16, 24, 8
    cost = torch.from_numpy(batch).to(dev)
    f64 = torch.full((3, b + 2 * g), -7.0, device=dev, dtype=torch.float64)
    bids = torch.full((b + 2 * g,), -7, device=dev, dtype=torch.int64)
    status = torch.full((b + 2 * g,), -7, device=dev, dtype=torch.int32)
    cols = torch.full((b * n + 2 * g,), -7, device=dev, dtype=torch.int32)
    rc = lib.sda_assignment_auction(cost.data_ptr(), n, b, 1e-7, 5, f64[0, g:].data_ptr(), f64[1, g:].data_ptr(), f64[2, g:].data_ptr(),
                                    bids[g:].data_ptr(), status[g:].data_ptr(), cols[g:].data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for t, count in ((f64[0], b), (f64[1], b), (f64[2], b), (bids, b), (status, b), (cols, b * n)):
        assert (t[:g] == -7).all() and (t[g + count:] == -7).all()
    assert status[g:g + b].tolist() == [A.NOT_CONVERGED] * 6 + [A.BADARG, A.NOT_CONVERGED] and (bids[g:g + b] <= 5).all()
    assert lib.sda_assignment_auction(cost.data_ptr(), 4097, 1, 1e-7, 5, f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(),
                                      bids.data_ptr(), status.data_ptr(), cols.data_ptr(), ops._stream()) == A.UNSUPPORTED


@pytest.mark.parametrize('n,offset', [(1024, 0), (1000, 0), (260, 1)])
def test_against_the_exact_solver(dev, n, offset):
    """n = 1024 (the evaluation's size), n = 1000 (no multiple of 64) and a view that starts one float into its buffer (rows not
    16-byte aligned: the dword loader at an n that is a multiple of 4)."""
    from sda_amd import ops
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    cost = torch.cdist(x.double(), y.double()).float()
    buf = torch.zeros(n * n + 4, device=dev)
    view = buf[offset:offset + n * n].view(n, n)
    view.copy_(cost)
    assert view.data_ptr() % 16 == 4 * offset
    got = device_auction(view, dev)
    total, cols = ops.assignment_cost(cost)
    exact = A.check_certificate(cost.numpy(), got, cols.numpy())
    assert abs(exact - total) <= 1e-12 * abs(total)
    assert int(got['bids']) <= ops.auction_default_budget(n)


@pytest.fixture()
def emd_state():
    from sda_amd import metrics
    saved = (metrics.EMD_SOLVER, metrics.EMD_BID_BUDGET, metrics.LAST_EMD_ROUTE)
    yield metrics
    metrics.EMD_SOLVER, metrics.EMD_BID_BUDGET, metrics.LAST_EMD_ROUTE = saved


def test_emd_routes(dev, emd_state, monkeypatch):
    from sda_amd import ops
    metrics = emd_state
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(257, 5, 3, generator=g).to(dev), (torch.randn(257, 5, 3, generator=g) * 1.5 + 0.3).to(dev)
    host = metrics.emd(x, y, solver='host')
    assert metrics.LAST_EMD_ROUTE == 'host'
    default = metrics.emd(x, y)                                                  # the default route is the host route, bit for bit
    assert metrics.LAST_EMD_ROUTE == 'host' and torch.equal(default, host) and default.dtype == x.dtype and default.device == x.device
    device = metrics.emd(x, y, solver='device')
    assert metrics.LAST_EMD_ROUTE == 'device'
    cost = ops.pairwise_dist(x.flatten(1), y.flatten(1), squared=False)
    eps_final = metrics.EMD_EPS_REL * float(cost.max() - cost.min())
    ulp = float(torch.finfo(torch.float32).eps) * float(host)                    # the fp32 rounding of either returned tensor
    print(f'emd host {float(host)!r} device {float(device)!r} eps_final {eps_final:.3e}')
    assert -ulp <= float(device) - float(host) <= eps_final + ulp
    # unequal counts: always the host flow solver
    assert torch.equal(metrics.emd(x, y[:200], solver='device'), metrics.emd(x, y[:200], solver='host'))
    assert metrics.LAST_EMD_ROUTE == 'host'
    metrics.emd(x, y[:200], solver='device')
    assert metrics.LAST_EMD_ROUTE == 'host'
    # a budget that cannot suffice: the host solver runs on the same cost matrix
    monkeypatch.setattr(metrics, 'EMD_BID_BUDGET', 300)
    assert torch.equal(metrics.emd(x, y, solver='device'), host) and metrics.LAST_EMD_ROUTE == 'host_fallback'
    monkeypatch.setattr(metrics, 'EMD_BID_BUDGET', None)
    # non-finite samples raise on both routes
    bad = x.clone()
    bad[7, 2, 1] = float('nan')
    for solver in ('host', 'device'):
        with pytest.raises(ops._lib.SdaHipError):
            metrics.emd(bad, y, solver=solver)


def test_install_as_sda_native_emd(dev, emd_state):
    import sys
    import sda_amd
    metrics = emd_state
    saved = {k: v for k, v in sys.modules.items() if k == 'sda' or k.startswith('sda.')}
    try:
        sda_amd.install_as_sda()
        assert metrics.EMD_SOLVER == 'host'                                      # the default stays the host solver
        sda_amd.install_as_sda(native_emd=True)
        assert metrics.EMD_SOLVER == 'device'
        from sda.utils import emd
        g = torch.Generator().manual_seed(5)
        x, y = torch.randn(64, 4, 3, generator=g).to(dev), torch.randn(64, 4, 3, generator=g).to(dev)
        got = emd(x, y)
        assert metrics.LAST_EMD_ROUTE == 'device'
        ref = metrics.emd(x, y, solver='host')
        assert abs(float(got) - float(ref)) <= 2e-7 * float(ref) + 1e-7 * 20
    finally:
        for k in [k for k in sys.modules if k == 'sda' or k.startswith('sda.')]:
            del sys.modules[k]
        sys.modules.update(saved)
