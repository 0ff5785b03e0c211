"""CPU: the domain-localised ensemble-space smoother (csrc/enks_local.hip).  The plan builder against the float64 one of
tests/enks_local_ref.py; that the cases cover the list lengths and that no bound is vacuous; the float64 replay's reduction to
``enks_wide_ref.analysis``; the host twins against the replay under the project's bound rule; locality and reproducibility,
bitwise; their refusals; the unchanged ABI; ``observe.positions``; and the routes of the experiment entries."""
import numpy as np
import pytest
import torch

from tests import enks_local_ref as R
from tests import enks_wide_ref as RW
from tests.chain_util import bound


def _plan(m, event, block, name, radius):
    return R.plan(event, R.positions(name, event), radius, block)


def test_the_cases_cover_the_list_lengths():
    lengths = set()
    for m, event, block, name, radius, sigmas in R.SHAPES:
        P = _plan(m, event, block, name, radius)
        lengths |= set(np.diff(P['offsets']).tolist())
        assert 1e-3 not in sigmas or R.full_rank(m, P), (m, event)
    print(sorted(lengths))
    assert {0, 1, 3, 4, 5} <= lengths and max(lengths) > 64
    assert {s[0] for s in R.SHAPES} == {2, 15, 17, 67, 128}


@pytest.mark.parametrize('m,event,block,name,radius,sigmas', R.SHAPES, ids=R.SHAPE_IDS)
def test_plan_matches_the_float64_builder(m, event, block, name, radius, sigmas):
    from sda_amd import ops
    P = _plan(m, event, block, name, radius)
    Q = ops.enkl_plan(event, R.positions(name, event), radius, block, device='cpu')
    assert Q.nblk == P['nblk'] and Q.k == len(R.positions(name, event))
    assert np.array_equal(Q.offsets_host, P['offsets']) and np.array_equal(Q.idx_host, P['idx'])
    assert Q.rho_host.dtype == np.float32 and Q.offsets_host.dtype == np.int32 and Q.idx_host.dtype == np.int32
    assert (Q.rho_host > 0).all()
    err, tol = np.abs(Q.rho_host.astype(np.float64) - P['rho']).max(), bound(R.plan32(event, R.positions(name, event), radius, block),
                                                                             P['rho'])
    print(f'rho: err {err:.3e} bound {tol:.3e}')
    assert err <= tol


def test_plan_on_a_ring_and_with_an_infinite_radius():
    from sda_amd import ops
    Q = ops.enkl_plan((40,), np.arange(0, 40, 2, dtype=np.float64), 2.0, 4, device='cpu')
    P = R.plan((1, 1, 40), R.positions('stride2', (1, 1, 40)), 2.0, (1, 4))
    assert Q.event == (1, 1, 40) and Q.block == (1, 4) and Q.nblk == 10
    assert np.array_equal(Q.offsets_host, P['offsets']) and np.array_equal(Q.idx_host, P['idx'])
    Q = ops.enkl_plan((2, 16, 16), R.positions('coarsen', (2, 16, 16)), float('inf'), (16, 16), device='cpu')
    assert Q.nblk == 1 and Q.offsets_host.tolist() == [0, 128] and (Q.rho_host == 1).all() and Q.idx_host.tolist() == list(range(128))
    # the periodic distance: the block at the end of the ring lists the observed value at its start
    Q = ops.enkl_plan((40,), [0.0], 2.0, 4, device='cpu')
    assert np.diff(Q.offsets_host).tolist() == [1] + [0] * 8 + [1]


def test_plan_refusals():
    from sda_amd import ops
    from sda_amd._lib import SdaHipError
    pos = R.positions('coarsen', (2, 16, 16))
    for bad in (dict(block=(5, 4)), dict(block=(4, 3)), dict(radius=0.0), dict(radius=-1.0), dict(radius=float('nan')),
                dict(positions=pos[:, 0]), dict(positions=np.zeros((4, 3))), dict(block=4)):
        kw = dict(event=(2, 16, 16), positions=pos, radius=2.0, block=(4, 4), device='cpu')
        kw.update(bad)
        with pytest.raises(SdaHipError):
            ops.enkl_plan(**kw)
    with pytest.raises(SdaHipError):
        ops.enkl_plan((40,), np.zeros((20, 3)), 2.0, 4, device='cpu')
    with pytest.raises(SdaHipError):
        ops.enkl_plan((40,), np.zeros(20), 2.0, 3, device='cpu')


@pytest.mark.parametrize('m,event,block,name,radius,window,inflation,sigma', R.CASES, ids=R.IDS)
def test_the_bound_of_a_case_is_not_vacuous(m, event, block, name, radius, window, inflation, sigma):
    """The fp32 replay must itself be close: a bound above 1e-4 of max|ref64| would let almost anything pass."""
    slabs, lo, t = window
    c = R.case(m, event, block, name, radius, slabs, lo, t, inflation, sigma)
    (S64, _, W64), (S32, _, W32) = c['ref64'], c['ref32']
    for nm, r32, r64 in (('S', S32[lo:t + 1], S64[lo:t + 1]), ('W', R.acting(W32, sigma), R.acting(W64, sigma))):
        tol = bound(r32, r64)
        print(f'{nm}: bound {tol:.3e} of max {np.abs(r64).max():.3e}')
        assert tol < 1e-4 * np.abs(r64).max()


REDUCTIONS = [(15, 48, 5, 'select', (1, 1, 48)), (17, 200, 300, 'select', (1, 1, 200)), (128, 512, 64, 'vortcoarse', (2, 16, 16))]


def reduction_plan(d, k, name, event):
    """One block over the whole grid with radius = inf: positions are irrelevant to the weights, any k finite pairs do."""
    return R.plan(event, np.zeros((k, 2)), float('inf'), event[1:])


@pytest.mark.parametrize('m,d,k,name,event', REDUCTIONS, ids=[f'M{r[0]}-d{r[1]}-k{r[2]}' for r in REDUCTIONS])
@pytest.mark.parametrize('inflation', R.INFLATIONS)
def test_one_block_with_an_infinite_radius_is_the_global_analysis(m, d, k, name, event, inflation):
    slabs, lo, t = R.WINDOWS[2]
    c = RW.case(m, d, k, name, slabs, lo, t, inflation, 1.0)
    P = reduction_plan(d, k, name, event)
    assert P['nblk'] == 1 and (P['rho'] == 1).all() and len(P['idx']) == k
    S64, _, W64 = R.analysis(c['S'], lo, t, c['A'], 1.0, c['y'], c['eps'], inflation, P, np.float64)
    err = np.abs(S64 - c['ref64'][0]).max()
    print(f'localised (one block, rho = 1) - global {err:.3e}')
    assert err <= 1e-9 * np.abs(c['S']).max()
    # and the host twins lie within the bound of the same reference as enks_wide's
    S = np.array(c['S'])
    assert RW.host_inflate(S, t, inflation) == 0
    H = np.ascontiguousarray(c['A'](S[t], np.float32), np.float32)
    w = R.host_weights(P, H, c['y'], 1.0, c['seed'], c['draw'])
    assert w['rcs'] == (0, 0, 0) and w['status'].tolist() == [0] and R.host_transform(P, S, lo, t, w['W']) == 0
    err, tol = np.abs(S[lo:t + 1] - c['ref64'][0][lo:t + 1]).max(), bound(c['ref32'][0][lo:t + 1], c['ref64'][0][lo:t + 1])
    print(f'S: err {err:.3e} bound {tol:.3e}')
    assert err <= tol


@pytest.mark.parametrize('m,event,block,name,radius,window,inflation,sigma', R.CASES, ids=R.IDS)
def test_host_twins_match_the_float64_replay(m, event, block, name, radius, window, inflation, sigma):
    slabs, lo, t = window
    c = R.case(m, event, block, name, radius, slabs, lo, t, inflation, sigma)
    S, H, w = R.host_analysis(c, lo, t, sigma, inflation)
    assert w['rcs'] == (0, 0, 0) and not w['status'].any()
    (S64, H64, W64), (S32, H32, W32) = c['ref64'], c['ref32']
    for nm, got, r32, r64 in (('W', R.acting(w['W'], sigma), R.acting(W32, sigma), R.acting(W64, sigma)), ('S', S[lo:t + 1], S32[lo:t + 1], S64[lo:t + 1])):
        err, tol = np.abs(got.astype(np.float64) - r64).max(), bound(r32, r64)
        print(f'{nm}: err {err:.3e} bound {tol:.3e} ratio {err / tol:.3f}')
        assert err <= tol, (nm, err, tol)
    outside = [s for s in range(slabs) if not lo <= s <= t]
    assert outside and all(np.array_equal(S[s], c['S'][s]) for s in outside)        # bitwise untouched
    assert np.array_equal(w['T'][:, :m], w['Y'].T) and np.array_equal(w['T'][:, m:], w['D'].T)


def test_an_empty_list_leaves_its_block_untouched():
    m, event, block, name, radius, _ = R.SHAPES[0]
    c = R.case(m, event, block, name, radius, 4, 1, 2, 1.0, 1.0)
    P = c['P']
    empty = np.nonzero(np.diff(P['offsets']) == 0)[0]
    assert len(empty) == 4
    S, H, w = R.host_analysis(c, 1, 2, 1.0, 1.0)
    for b in range(P['nblk']):
        same = np.array_equal(S[:, :, P['comps'][b]], c['S'][:, :, P['comps'][b]])
        assert same == (b in empty) and bool(w['W'][b].any()) != (b in empty)


@pytest.mark.parametrize('shape', [R.SHAPES[1], R.SHAPES[6]], ids=[R.SHAPE_IDS[1], R.SHAPE_IDS[6]])
def test_an_observation_reaches_only_the_blocks_that_list_it(shape):
    m, event, block, name, radius, _ = shape
    slabs, lo, t = R.WINDOWS[1]
    c = R.case(m, event, block, name, radius, slabs, lo, t, 1.0, 1.0)
    P = c['P']
    i0 = int(P['idx'][len(P['idx']) // 2])
    listing = R.blocks_listing(P, i0)
    assert 0 < len(listing) < P['nblk']
    base = R.host_analysis(c, lo, t, 1.0, 1.0)
    for value in (float(c['y'][i0]) + 1.0, np.inf):
        y = np.array(c['y'])
        y[i0] = value
        S, H, w = R.host_analysis(c, lo, t, 1.0, 1.0, y=y)
        assert w['status'].tolist() == [int(not np.isfinite(value) and b in listing) for b in range(P['nblk'])]
        for b in range(P['nblk']):
            comp = P['comps'][b]
            if b not in listing:
                assert np.array_equal(w['W'][b], base[2]['W'][b]) and np.array_equal(S[:, :, comp], base[0][:, :, comp])
            elif np.isfinite(value):
                assert not np.array_equal(w['W'][b], base[2]['W'][b]) and not np.array_equal(S[:, :, comp], base[0][:, :, comp])
            else:
                assert not w['W'][b].any() and np.array_equal(S[:, :, comp], c['S'][:, :, comp])


def test_reproducible_and_independent_of_the_other_slabs():
    m, event, block, name, radius, _ = R.SHAPES[8]
    slabs, lo, t = R.WINDOWS[2]
    c = R.case(m, event, block, name, radius, slabs, lo, t, 1.05, 1.0)
    first, again = R.host_analysis(c, lo, t, 1.0, 1.05), R.host_analysis(c, lo, t, 1.0, 1.05)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[2]['W'], again[2]['W'])
    shorter = R.host_analysis(c, t - 1, t, 1.0, 1.05)
    assert np.array_equal(first[0][t - 1:t + 1], shorter[0][t - 1:t + 1]) and np.array_equal(shorter[0][:t - 1], c['S'][:t - 1])


def test_a_stray_index_flags_its_block_and_is_not_read():
    m, event, block, name, radius, _ = R.SHAPES[1]
    c = R.case(m, event, block, name, radius, 4, 1, 2, 1.0, 1.0)
    P = dict(c['P'])
    P['idx'] = np.array(P['idx'])
    P['idx'][4] = c['k']                                                          # block 1's second entry
    S, H, w = R.host_analysis(c, 1, 2, 1.0, 1.0)
    bad = R.host_weights(P, H, c['y'], 1.0, c['seed'], c['draw'])
    assert bad['status'].tolist() == [0, 1] + [0] * 8 and not bad['W'][1].any()
    assert np.array_equal(np.delete(bad['W'], 1, 0), np.delete(w['W'], 1, 0))


@pytest.mark.parametrize('host', [True, False], ids=['host-twins', 'device-entries'])
def test_refusals_before_anything_runs(host):
    """Every entry refuses on the host, before a launch or a memory access: the pointers here are not mapped."""
    from sda_amd import _lib
    lib = R.emu() if host else _lib.load()
    P = 0x10000
    sfx, tail = ('_host', ()) if host else ('', (None,))
    pack, weights, tr = (getattr(lib, f'sda_enkl_{n}{sfx}') for n in ('pack', 'weights', 'transform'))
    assert pack(P, P, 129, 4, P, *tail) == -2 and pack(P, P, 1, 4, P, *tail) == -2 and pack(P, P, 8, 0, P, *tail) == -1
    assert pack(None, P, 8, 4, P, *tail) == -1 and pack(P, P, 8, 4, None, *tail) == -1
    ok = [P, 8, 4, P, P, P, 3, 1.0, P, P, P]
    for pos, value, rc in ((1, 129, -2), (1, 1, -2), (1, 0, -1), (2, 0, -1), (6, 0, -1), (6, (1 << 22) + 1, -2), (7, 0.0, -1), (0, None, -1),
                           (3, None, -1), (4, None, -1), (5, None, -1), (8, None, -1), (9, None, -1), (10, None, -1)):
        args = list(ok)
        args[pos] = value
        assert weights(*args, *tail) == rc, (pos, value)
    ok = [P, 8 * 512, 512, 1, 8, 2, 16, 16, 4, 4, P, P]
    for pos, value, rc in ((4, 129, -2), (4, 1, -2), (3, 65536, -2), (3, 0, -1), (8, 5, -1), (9, 3, -1), (2, 511, -1), (1, -1, -1),
                           (0, None, -1), (10, None, -1), (11, None, -1), (5, 0, -1), (8, 0, -1)):
        args = list(ok)
        args[pos] = value
        assert tr(*args, *tail) == rc, (pos, value)


def test_abi_14_is_unchanged_and_the_new_symbols_resolve():
    from sda_amd import _lib
    lib = _lib.load()
    assert lib.sda_abi_version() == 14
    names = ['sda_enkl_pack', 'sda_enkl_weights', 'sda_enkl_transform']
    assert all(n in _lib.SIGNATURES and getattr(lib, n) is not None for n in names)
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.__file__)), 'include', 'sda_hip.h')) as f:
        header = f.read()
    assert all(f' {n}(' in header for n in names) and 'Gaspari-Cohn' in header


def test_ops_check_their_arguments_without_a_device():
    from sda_amd import chains, ops
    from sda_amd._lib import SdaHipError
    plan = ops.enkl_plan((40,), np.arange(0, 40, 2.0), 2.0, 4, device='cpu')
    with pytest.raises(SdaHipError):
        ops.enkl_weights(plan, torch.zeros(4, 20), torch.zeros(4, 20), 1.0)     # CPU tensors: no fallback
    with pytest.raises(SdaHipError):
        ops.enkl_transform(plan, torch.zeros(2, 4, 40), 0, 1, torch.zeros(10, 4, 4))
    with pytest.raises(SdaHipError):
        chains.enks_local(None, torch.zeros(4, 40), torch.zeros(1, 20), lambda x: x[..., ::2], 1.0, positions=np.arange(0, 40, 2.0),
                          radius=2.0, block=4)


def test_positions_of_the_observe_operators():
    from sda_amd import observe
    from sda_amd._lib import SdaHipError
    p = observe.positions(observe.Coarsen(2), (2, 16, 16))
    assert p.shape == (128, 2) and p.dtype == np.float64
    assert np.array_equal(p, np.array([(2 * i + 0.5, 2 * j + 0.5) for _ in range(2) for i in range(8) for j in range(8)]))
    p = observe.positions(observe.Subsample.space(4, 1), (2, 16, 16))
    assert np.array_equal(p, np.array([(float(i), float(j)) for _ in range(2) for i in (1, 5, 9, 13) for j in (1, 5, 9, 13)]))
    p = observe.positions(observe.Crop((slice(2, 4), slice(14, 16))), (1, 16, 16))
    assert np.array_equal(p, np.array([(2.0, 14.0), (2.0, 15.0), (3.0, 14.0), (3.0, 15.0)]))
    p = observe.positions(observe.Compose(observe.Vorticity(), observe.Coarsen(4), observe.Pointwise('saturate')), (2, 16, 16))
    assert np.array_equal(p, np.array([(4 * i + 1.5, 4 * j + 1.5) for i in range(4) for j in range(4)]))
    p = observe.positions(observe.Subsample((slice(0, None, 2),)), (8,))
    assert np.array_equal(p, np.array([(0.0, 0.0), (0.0, 2.0), (0.0, 4.0), (0.0, 6.0)]))
    for name, event in (('stride2', (3, 12, 20)), ('coarsen', (3, 12, 20)), ('satcoarsen', (2, 16, 16)), ('stride2', (1, 1, 40))):
        op = R.device_operator(name, event)[0]
        assert np.array_equal(observe.positions(op, event if event[1] > 1 else event[2:]), R.positions(name, event))
    for bad in (lambda x: x, observe.TimeDiff(), observe.Select(-1, 0)):
        with pytest.raises(SdaHipError):
            observe.positions(bad, (2, 16, 16))


def test_the_routes_of_the_experiment_entries(monkeypatch):
    """radius=None calls what was called before; a number calls ``chains.enks_local`` with the positions."""
    from sda_amd import chains, observe
    from sda_amd.experiments import kolmogorov, lorenz
    calls = []

    class Chain:
        def __init__(self, event):
            self.event = event

        def prior(self, shape, device=None, **kw):
            return torch.zeros(*shape, *self.event)

        def trajectory(self, x, length, last=False, **kw):
            return x

    def wide(chain, x, y, A, sigma, step, **kw):
        calls.append(('wide', A, kw))
        return torch.zeros(x.shape[0], len(y) * step + 1, *x.shape[1:])

    def local(chain, x, y, A, sigma, step, **kw):
        calls.append(('local', A, kw))
        return torch.zeros(x.shape[0], len(y) * step + 1, *x.shape[1:])

    monkeypatch.setattr(chains, 'enks_wide', wide)
    monkeypatch.setattr(chains, 'enks_local', local)
    A = lambda x: x[..., ::2]  # noqa: E731
    y = torch.zeros(3, 4)
    common = dict(lag=1, inflation=1.05, seed=1)
    lorenz.enks(y, A, 0.5, 2, 8, chain=Chain((8,)), burn=0, device='cpu', space='ensemble', **common)
    assert calls == [('wide', A, common)]
    del calls[:]
    out = lorenz.enks(y, A, 0.5, 2, 8, chain=Chain((8,)), burn=0, device='cpu', space='ensemble', radius=2.0, block=2, **common)
    assert calls[0][0] == 'local' and calls[0][1] is A and out.shape == (8, 5, 8)
    kw = dict(calls[0][2])
    assert list(kw.pop('positions')) == [0.0, 2.0, 4.0, 6.0] and kw == dict(radius=2.0, block=2, **common)
    del calls[:]
    lorenz.enks(y, lambda x: x[..., ::2] ** 2, 0.5, 2, 8, chain=Chain((8,)), burn=0, device='cpu', space='ensemble', radius=2.0,
                positions=[0.0, 2.0, 4.0, 6.0], **common)
    assert calls[0][0] == 'local' and calls[0][2]['block'] == 4
    with pytest.raises(chains.SdaHipError):
        lorenz.enks(y, lambda x: x[..., ::2] + x[..., 1::2], 0.5, 2, 8, chain=Chain((8,)), burn=0, device='cpu', space='ensemble', radius=2.0)
    with pytest.raises(ValueError):
        lorenz.enks(y, A, 0.5, 2, 8, chain=Chain((8,)), burn=0, device='cpu', radius=2.0)
    del calls[:]
    C2 = observe.Coarsen(2)
    yk = torch.zeros(3, 2, 4, 4)
    kolmogorov.enks(yk, C2, 0.5, 2, 8, chain=Chain((2, 8, 8)), device='cpu', **common)
    assert calls == [('wide', C2, common)]
    del calls[:]
    kolmogorov.enks(yk, C2, 0.5, 2, 8, chain=Chain((2, 8, 8)), device='cpu', radius=3.0, **common)
    kw = dict(calls[0][2])
    assert calls[0][0] == 'local' and np.array_equal(kw.pop('positions'), observe.positions(C2, (2, 8, 8)))
    assert kw == dict(radius=3.0, block=(4, 4), **common)
