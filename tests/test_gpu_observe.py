"""GPU: the observation operators of sda_amd/csrc/observe.hip (sda_amd.observe) against the float64 index-list reference
of tests/observe_ref.py: odd slice layouts, guard bands around every output, tensors past the launch-grid cap, views that
are not contiguous, the one-launch guidance against its formula, edge geometry, and adjointness as an identity.

Grid sizing.  Every launcher in observe.hip sizes its grid with obs_grid(total) = min(ceil(total / 256), 65536) blocks of 256
threads (mask and timediff included: there is no entry with an uncapped grid), and every kernel walks
``i += gridDim.x * blockDim.x`` in 64-bit arithmetic.  A thread therefore runs a second iteration once ``total`` exceeds
65536 * 256 = 16 777 216, where ``total`` is the entry's own loop count:

    entry point                  loop count (cap at 16 777 216)   reached by
    sda_obs_subsample            output elements                  subsample_table, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_subsample (x[..., 1:], 17.2 M outputs; space(4) gives
                                                                  1.1 M outputs and stays in the first iteration)
    sda_obs_subsample_adjoint    input (x) elements               subsample_table, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_subsample
    sda_obs_subsample_guidance   input (x) elements               subsample_table, fused_guidance*, guard_band, noncontiguous,
                                                                  past_cap_guidance
    sda_obs_coarsen              output elements                  edge_coarsen, guard_band, noncontiguous, adjoint_identity
                                                                  (no large case: a 17 M output needs a 276 M input at f = 4)
    sda_obs_coarsen_adjoint      input elements                   edge_coarsen, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_coarsen_adjoint
    sda_obs_vorticity            output elements = input / 2      edge_vorticity, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_vorticity (a 34.6 M input)
    sda_obs_vorticity_adjoint    cotangent elements = output / 2  the same; past_cap_vorticity (a 17.3 M cotangent)
    sda_obs_pointwise            elements                         pointwise_*, guard_band, noncontiguous, past_cap_pointwise
    sda_obs_pointwise_vjp        elements                         pointwise_*, nonlinear_adjoint_identity, guard_band,
                                                                  noncontiguous, past_cap_pointwise
    sda_obs_mask                 elements                         edge_mask, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_mask
    sda_obs_timediff             output elements = input / len    edge_timediff, guard_band, noncontiguous, adjoint_identity,
                                                                  past_cap_timediff (len 2 on a 34.6 M input)
    sda_obs_timediff_adjoint     input elements                   the same; past_cap_timediff

(include/sda_hip.h declares these twelve sda_obs_* entries.)  The indices stay far below 2^31, so these cases see a wrong
stride, a dropped loop or a wrong per-iteration decomposition, not a 32-bit loop variable, which differs only past 2^31
elements.

Tolerances.  Gather, scatter, select, mask and timediff do at most one float32 operation per value: torch.equal with the
float32-rounded reference.  Coarsen, vorticity, pointwise and the guidance formula do a handful; their bound is four times the
largest scale-relative error measured on an MI355X over the cases of this file, clamped to [2e-7, 1e-5]:

    family             measured max error      bound
    coarsen            2.03e-7  (6 x 12 plane, f = 6)            8.2e-7
    vorticity          7.92e-8  (3 x 3 grid)                     3.2e-7
    pointwise          1.74e-7  (saturate VJP, 17.3 M elements)  7.0e-7
    guidance           1.45e-7  (17.3 M elements)                5.8e-7
    adjoint identity   2.48e-8  (frames(4) >> Coarsen(8))        2e-7 (the floor; 4 x measured = 9.9e-8)
                       as |<Ax, r> - <x, A^T r>| / sqrt(<Ax, Ax> <r, r>); the non-linear members stay inside the
                       finite-difference bound alone (excess 0 to 9.5e-10)

Every tolerance comparison prints its figure (``OBSERVE-ERR family case value``) before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import observe_ref as R
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

TOL = {'coarsen': 8.2e-7, 'vorticity': 3.2e-7, 'pointwise': 7.0e-7, 'guidance': 5.8e-7, 'identity': 2e-7}
S = slice
I5 = ctypes.c_int * 5
GUARD = 64
# float32-representable, so that the float64 formula sees the numbers the kernel sees
STD, GAMMA, MU, SIGMA = 0.375, 0.015625, 0.8125, 0.59375


@pytest.fixture(scope='module')
def dev():
    from sda_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _sid(v):
    return str(v).replace('slice', 's').replace('None', '').replace(' ', '')


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _t(a):
    a = np.asarray(a)
    return torch.from_numpy(a if a.flags.c_contiguous else a.copy(order='C'))


def _exact(got, ref, what):
    """got == the float32-rounded reference, bit for bit up to the sign of zero."""
    ref = _t(ref).float()
    assert tuple(got.shape) == tuple(ref.shape), f'{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.equal(got.cpu(), ref), f'{what}: differs from the float32-rounded reference'


def _close(got, ref, family, what):
    ref = _t(ref)
    print(f'OBSERVE-ERR {family} {what} {rel_err(got, ref) if ref.numel() else 0.0:.3e}')
    assert_close(got.cpu(), ref, TOL[family], what=what)


# ---------------------------------------------------------------------------------------------------------- Subsample table
SUBSAMPLE = [
    # one, two, three, four and five sliced dims; steps that do not divide the extent
    ((13, 11, 7), (S(None, None, 3),)),
    ((13, 11, 7), (S(None, None, 4), S(1, None, 3))),
    ((5, 13, 11, 7), (S(2, None, 5), S(None), S(None, None, 2))),
    ((3, 2, 13, 11, 7), (S(None, None, 2), S(7, 12, 2), S(3, 10, 4), S(None, None, 3))),   # starts past a step, with stops
    ((2, 3, 5, 11, 7), (S(None), S(1, None, 2), S(None, None, 2), S(5, 10, 3), S(None, -1))),
    ((1, 1, 2, 3, 5, 11, 7), (S(1, None), S(None, None, 2), S(0, 4, 3), S(2, 9, 5), S(3, None, 3))),   # five, behind 1s
    # negative starts and stops
    ((13, 11, 7), (S(-5, None, 2),)),
    ((13, 11, 7), (S(None, -1), S(None, -1))),
    ((13, 11, 7), (S(-9, -2, 3), S(-6, None, 4))),
    # a step as large as, or larger than, the extent
    ((13, 11, 7), (S(None, None, 11), S(None, None, 20))),
    ((13, 11, 7), (S(4, None, 20), S(6, None, 9))),
    # no leading dims; a single dim; several leading dims folded into one; no sliced dim at all
    ((11, 7), (S(None, None, 4), S(1, None, 3))),
    ((7,), (S(1, None, 3),)),
    ((37,), (S(35, None, 5),)),
    ((2, 2, 2, 13, 11, 7), (S(None, None, 4), S(1, 6, 2))),
    ((13, 11, 7), ()),
    ((4, 13, 11), (S(5, 6), S(None))),
    ((3, 65, 3), (S(None, None, 8), S(0, 1))),
]
SUBSAMPLE_EMPTY = [
    ((13, 11, 7), (S(10, 4), S(None))),                 # start past the stop
    ((13, 11, 7), (S(3, 3),)),
    ((13, 11, 7), (S(None), S(20, None, 2))),           # start past the extent
    ((11, 7), (S(None, None, 2), S(-1, -3))),
]


@pytest.mark.parametrize('shape,slices', SUBSAMPLE, ids=_sid)
def test_subsample_table(dev, shape, slices):
    from sda_amd import observe as Ob
    op, ref = Ob.Subsample(slices), R.subsample(shape, slices)
    x = _randn(shape, 1)
    assert op.out_shape(shape) == ref.out_shape
    _exact(op(x.to(dev)), ref.forward(x.numpy()), 'forward')
    r = _randn(ref.out_shape, 2)
    g = op.adjoint(r.to(dev), shape)
    _exact(g, ref.adjoint(r.numpy()), 'adjoint')
    eps, y = _randn(shape, 3), _randn(ref.out_shape, 4)
    gg = op.gaussian_guidance(x.to(dev), eps.to(dev), y.to(dev), STD, GAMMA, MU, SIGMA)
    assert gg is not None
    want = R.gaussian_guidance(ref, x.numpy(), eps.numpy(), y.numpy(), STD, GAMMA, MU, SIGMA)
    _close(gg, want, 'guidance', f'guidance {shape} {slices}')
    unobserved = _t(ref.adjoint(np.ones(ref.out_shape))) == 0
    assert not gg.cpu()[unobserved].any(), 'guidance is not zero off the observed lattice'


@pytest.mark.parametrize('shape,slices', SUBSAMPLE_EMPTY, ids=_sid)
def test_subsample_empty_result(dev, shape, slices):
    """A slice that selects nothing: out_shape and the call agree with torch indexing, the adjoint and the guidance are the
    zero gradient that autograd through the indexing gives."""
    from sda_amd import observe as Ob
    op = Ob.Subsample(slices)
    x = _randn(shape, 1)
    want = x[(Ellipsis,) + tuple(slices)]
    assert want.numel() == 0
    assert op.out_shape(shape) == tuple(want.shape) == R.subsample(shape, slices).out_shape
    out = op(x.to(dev))
    assert tuple(out.shape) == tuple(want.shape) and out.dtype == torch.float32
    g = op.adjoint(torch.empty(want.shape, device=dev), shape)
    assert tuple(g.shape) == shape and g.dtype == torch.float32 and not g.any()
    ax, vjp = op.linearize(x.to(dev))
    assert tuple(ax.shape) == tuple(want.shape) and not vjp(ax).any()
    gg = op.gaussian_guidance(x.to(dev), x.to(dev), torch.empty(want.shape, device=dev), STD, GAMMA, MU, SIGMA)
    assert gg is not None and tuple(gg.shape) == shape and not gg.any()


# --------------------------------------------------------------------------------------------------------------- guard band
class _Guarded:
    """[64 NaN][payload, NaN-filled too][64 NaN]: the C entry gets the payload's address."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def check(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert b[:GUARD].isnan().all(), f'{what}: wrote in front of the output'
        assert b[GUARD + self.n:].isnan().all(), f'{what}: wrote past the end of the output'
        assert not b[GUARD:GUARD + self.n].isnan().any(), f'{what}: left output elements unwritten'
        return b[GUARD:GUARD + self.n]


def _guard_cases():
    size, start, step, stop = [1, 3, 5, 11, 13], [0, 0, 1, 1, 0], [1, 1, 2, 1, 2], [1, 3, 5, 10, 13]
    osize = [len(range(a, b, c)) for a, b, c in zip(start, stop, step)]
    nx, no = int(np.prod(size)), int(np.prod(osize))
    sl = lambda: (I5(*size), I5(*start), I5(*step), I5(*stop))
    # name -> (input element counts, output element count, call(lib, inputs, out_ptr))
    return {
        'sda_obs_subsample': ([nx], no, lambda lib, a, o: lib.sda_obs_subsample(a[0], *sl(), o, None)),
        'sda_obs_subsample_adjoint': ([no], nx, lambda lib, a, o: lib.sda_obs_subsample_adjoint(a[0], *sl(), o, None)),
        'sda_obs_subsample_guidance': ([nx, nx, no // 3], nx, lambda lib, a, o: lib.sda_obs_subsample_guidance(
            a[0], a[1], a[2], no // 3, *sl(), STD, GAMMA, MU, SIGMA, None, o, None)),
        'sda_obs_coarsen': ([5 * 9 * 15], 5 * 3 * 5, lambda lib, a, o: lib.sda_obs_coarsen(a[0], 5, 9, 15, 3, o, None)),
        'sda_obs_coarsen_adjoint': ([5 * 3 * 5], 5 * 9 * 15, lambda lib, a, o: lib.sda_obs_coarsen_adjoint(a[0], 5, 9, 15, 3, o, None)),
        'sda_obs_vorticity': ([3 * 2 * 9 * 11], 3 * 9 * 11, lambda lib, a, o: lib.sda_obs_vorticity(a[0], 3, 9, 11, o, None)),
        'sda_obs_vorticity_adjoint': ([3 * 9 * 11], 3 * 2 * 9 * 11, lambda lib, a, o: lib.sda_obs_vorticity_adjoint(a[0], 3, 9, 11, o, None)),
        'sda_obs_pointwise': ([601], 601, lambda lib, a, o: lib.sda_obs_pointwise(a[0], 601, 1, o, None)),
        'sda_obs_pointwise_vjp': ([601, 601], 601, lambda lib, a, o: lib.sda_obs_pointwise_vjp(a[0], a[1], 601, 1, o, None)),
        'sda_obs_mask': ([5 * 119, 119], 5 * 119, lambda lib, a, o: lib.sda_obs_mask(a[0], 5 * 119, a[1], 119, o, None)),
        'sda_obs_timediff': ([7 * 5 * 13], 7 * 13, lambda lib, a, o: lib.sda_obs_timediff(a[0], 7, 5, 13, 3, 1, o, None)),
        'sda_obs_timediff_adjoint': ([7 * 13], 7 * 5 * 13, lambda lib, a, o: lib.sda_obs_timediff_adjoint(a[0], 7, 5, 13, 3, 1, o, None)),
    }


def test_guard_cases_name_every_entry():
    from sda_amd import _lib
    assert set(_guard_cases()) == {n for n in _lib.SIGNATURES if n.startswith('sda_obs_')}


@pytest.mark.parametrize('entry', sorted(_guard_cases()))
def test_guard_band(dev, entry):
    """Each C entry writes every element of its output and nothing on either side of it."""
    from sda_amd import _lib
    lib = _lib.load()
    in_counts, n_out, call = _guard_cases()[entry]
    with torch.cuda.device(dev):
        ins = [_randn((n,), 10 + k).to(dev) for k, n in enumerate(in_counts)]
        out = _Guarded(n_out, dev)
        torch.cuda.synchronize()
        assert call(lib, [t.data_ptr() for t in ins], out.ptr) == 0
        out.check(entry)


# ------------------------------------------------------------------------------------------------------ past the grid cap
BIG = (2, 33, 2, 512, 256)            # 17 301 504 elements > 65536 * 256
TAIL = 4096


@pytest.fixture(scope='module')
def big(dev):
    x = _randn(BIG, 20)
    assert x.numel() > 65536 * 256
    return x, x.to(dev)


def _big_exact(got, ref, what):
    got, ref = got.cpu(), _t(ref)
    assert got.dtype == ref.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape), what
    assert torch.equal(got.reshape(-1)[-TAIL:], ref.reshape(-1)[-TAIL:]), f'{what}: the last {TAIL} elements differ'
    assert torch.equal(got, ref), what


def _big_close(got, ref, family, what):
    got, ref = got.cpu(), _t(ref)
    _close(got.reshape(-1)[-TAIL:], ref.reshape(-1)[-TAIL:].numpy(), family, f'{what} (last {TAIL})')
    _close(got, ref.numpy(), family, what)


def test_past_cap_subsample(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    for slices in ((S(None, None, 4), S(None, None, 4)), (S(1, None),)):        # 1.1 M and 17.2 M outputs
        op = Ob.Subsample(slices)
        out = op(xd)
        _big_exact(out, R.subsample_dense(x.numpy(), slices), f'forward {slices}')
        _big_exact(op.adjoint(out, BIG), R.subsample_adjoint_dense(out.cpu().numpy(), BIG, slices), f'adjoint {slices}')


def test_past_cap_guidance(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    slices = (S(None, None, 4), S(None, None, 4))
    op, ref = Ob.Subsample(slices), R.subsample(BIG, slices)
    eps = x.flip(0)
    y = _randn(ref.out_shape[1:], 21)
    g = op.gaussian_guidance(xd, xd.flip(0), y.to(dev), STD, GAMMA, MU, SIGMA)
    _big_close(g, R.gaussian_guidance(ref, x.numpy(), eps.numpy(), y.numpy(), STD, GAMMA, MU, SIGMA), 'guidance', 'guidance')


def test_past_cap_coarsen_adjoint(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    r = x[..., ::4, ::4].contiguous()
    _big_close(Ob.Coarsen(4).adjoint(r.to(dev), BIG), R.coarsen_adjoint_dense(r.double().numpy(), 4), 'coarsen', 'coarsen adjoint')


def test_past_cap_vorticity(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    xv = torch.stack([x, x.flip(-1)], dim=-3)                                    # (2, 33, 2, 2, 512, 256): 17.3 M outputs
    _big_close(Ob.Vorticity()(torch.stack([xd, xd.flip(-1)], dim=-3)), R.vorticity_dense(xv.numpy()), 'vorticity', 'vorticity')
    _big_close(Ob.Vorticity().adjoint(xd, xv.shape), R.vorticity_adjoint_dense(x.numpy()), 'vorticity', 'vorticity adjoint')


def test_past_cap_pointwise(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    ref = R.Pointwise(BIG, 'saturate')
    out, vjp = Ob.Pointwise('saturate').linearize(xd)
    _big_close(out, ref.forward(x.numpy()), 'pointwise', 'saturate')
    _big_close(vjp(xd.flip(0)), ref.linearize(x.numpy())[1](x.flip(0).numpy()), 'pointwise', 'saturate vjp')


def test_past_cap_mask(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    m = (_randn(BIG[-2:], 22) > 0).float() * 0.75
    _big_exact(Ob.Mask(m)(xd), x.numpy() * m.numpy(), 'mask')


def test_past_cap_timediff(dev, big):
    from sda_amd import observe as Ob
    x, xd = big
    xv = torch.stack([x, x.flip(-1)], dim=-3)                                    # len 2 along dim 3: 17.3 M outputs
    _big_exact(Ob.TimeDiff(3, 1, 0)(torch.stack([xd, xd.flip(-1)], dim=-3)), R.timediff_dense(xv.numpy(), 3, 1, 0), 'timediff')
    r = x[:, 5].contiguous()
    _big_exact(Ob.TimeDiff(1, 0, -1).adjoint(r.to(dev), BIG), R.timediff_adjoint_dense(r.numpy(), BIG, 1, 0, -1), 'timediff adjoint')


# --------------------------------------------------------------------------------------------------- non-contiguous inputs
def _transposed(shape, seed, dev):
    """A tensor of this shape that is a transpose view (first and last dim swapped) of a contiguous buffer."""
    base = list(shape)
    base[0], base[-1] = base[-1], base[0]
    t = _randn(base, seed).to(dev).transpose(0, -1)
    assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
    return t


LINEAR_NAMES = ['subsample', 'crop', 'select', 'coarsen', 'vorticity', 'mask', 'timediff', 'cell9 frames + coarsen',
                'cell16 coarsen + crop', 'cell4 masked vorticity', 'lorenz x[..., ::8, :1]']
NONLINEAR_NAMES = ['saturate', 'tanh', 'square', 'abs', 'cell23 saturating sensor']


def test_case_lists_are_complete():
    assert sorted(LINEAR_NAMES) == sorted(_linear_cases()) and sorted(NONLINEAR_NAMES) == sorted(_nonlinear_cases())


def _linear_cases():
    """name -> (x shape, sda_amd operator factory, reference factory(in_shape), exact?, family)"""
    from sda_amd import observe as Ob
    m = (_randn((6, 8), 30) > 0).float() * 0.5
    sl = (S(1, None, 2), S(None, -1, 3))
    return {
        'subsample': ((3, 5, 2, 6, 8), lambda: Ob.Subsample(sl), lambda s: R.subsample(s, sl), True, None),
        'crop': ((3, 5, 2, 6, 8), lambda: Ob.Crop((S(1, 5), S(2, 7))), lambda s: R.subsample(s, (S(1, 5), S(2, 7))), True, None),
        'select': ((3, 5, 2, 6, 8), lambda: Ob.Select(-4, -2), lambda s: R.select(s, -4, -2), True, None),
        'coarsen': ((3, 5, 2, 6, 8), lambda: Ob.Coarsen(2), lambda s: R.coarsen(s, 2), False, 'coarsen'),
        'vorticity': ((3, 5, 2, 6, 8), lambda: Ob.Vorticity(), R.vorticity, False, 'vorticity'),
        'mask': ((3, 5, 2, 6, 8), lambda: Ob.Mask(m), lambda s: R.mask(s, m.numpy()), True, None),
        'timediff': ((3, 5, 2, 6, 8), lambda: Ob.TimeDiff(1, 0, -1), lambda s: R.timediff(s, 1, 0, -1), True, None),
        # the chains of the reference's notebooks (figures.ipynb cells 9, 16, 4) at a 16 x 16 grid, and the Lorenz observation
        'cell9 frames + coarsen': ((2, 9, 2, 16, 16), lambda: Ob.Compose(Ob.Subsample.frames(4), Ob.Coarsen(8)),
                                   lambda s: R.Chain(s, lambda q: R.subsample(q, (S(None, None, 4), S(None), S(None), S(None))),
                                                     lambda q: R.coarsen(q, 8)), False, 'coarsen'),
        'cell16 coarsen + crop': ((2, 9, 2, 16, 16),
                                  lambda: Ob.Compose(Ob.Coarsen(4), Ob.Crop((S(None, None, 3), S(None), S(1, 3), S(1, 3)))),
                                  lambda s: R.Chain(s, lambda q: R.coarsen(q, 4),
                                                    lambda q: R.subsample(q, (S(None, None, 3), S(None), S(1, 3), S(1, 3)))),
                                  False, 'coarsen'),
        'cell4 masked vorticity': ((2, 9, 2, 6, 8), lambda: Ob.Compose(Ob.Select(-4, -1), Ob.Vorticity(), Ob.Mask(m)),
                                   lambda s: R.Chain(s, lambda q: R.select(q, -4, -1), R.vorticity, lambda q: R.mask(q, m.numpy())),
                                   False, 'vorticity'),
        'lorenz x[..., ::8, :1]': ((3, 65, 3), lambda: Ob.Subsample((S(None, None, 8), S(0, 1))),
                                   lambda s: R.subsample(s, (S(None, None, 8), S(0, 1))), True, None),
    }


def _cmp(got, ref, exact, family, what):
    if exact:
        _exact(got, ref, what)
    else:
        _close(got, ref, family, what)


@pytest.mark.parametrize('name', LINEAR_NAMES)
def test_noncontiguous_linear(dev, name):
    """Transpose views in: the same bits out as for the contiguous copy, for the call, the adjoint and linearize."""
    shape, make, make_ref, exact, family = _linear_cases()[name]
    op, ref = make(), make_ref(shape)
    xt = _transposed(shape, 31, dev)
    out = op(xt)
    assert torch.equal(out, op(xt.contiguous()))
    _cmp(out, ref.forward(xt.cpu().numpy()), exact, family, name)
    rt = _transposed(ref.out_shape, 32, dev)
    g = op.adjoint(rt, shape)
    assert torch.equal(g, op.adjoint(rt.contiguous(), shape))
    _cmp(g, ref.adjoint(rt.cpu().numpy()), exact, family, name + ' adjoint')
    ax, vjp = op.linearize(xt)
    assert torch.equal(ax, out) and torch.equal(vjp(rt), g)


@pytest.mark.parametrize('kind', ['saturate', 'tanh', 'square', 'abs'])
def test_noncontiguous_pointwise(dev, kind):
    from sda_amd import observe as Ob
    shape = (5, 7, 33)                                                           # 1155 elements: five blocks, the last partial
    op, ref = Ob.Pointwise(kind), R.Pointwise(shape, kind)
    xt, rt = _transposed(shape, 33, dev) * 1.5, _transposed(shape, 34, dev)
    out, vjp = op.linearize(xt)
    out_c, vjp_c = op.linearize(xt.contiguous())
    assert torch.equal(out, out_c) and torch.equal(op(xt), out) and torch.equal(vjp(rt), vjp_c(rt.contiguous()))
    want, want_vjp = ref.linearize(xt.cpu().numpy())
    _close(out, want, 'pointwise', kind)
    _close(vjp(rt), want_vjp(rt.cpu().numpy()), 'pointwise', kind + ' vjp')


def test_noncontiguous_guidance(dev):
    from sda_amd import observe as Ob
    shape, sl = (4, 9, 3), (S(1, None, 4), S(None, 2))
    op, ref = Ob.Subsample(sl), R.subsample(shape, sl)
    xt, et = _transposed(shape, 35, dev), _transposed(shape, 36, dev)
    yt = _transposed(ref.out_shape, 37, dev)
    g = op.gaussian_guidance(xt, et, yt, STD, GAMMA, MU, SIGMA)
    assert torch.equal(g, op.gaussian_guidance(xt.contiguous(), et.contiguous(), yt.contiguous(), STD, GAMMA, MU, SIGMA))
    _close(g, R.gaussian_guidance(ref, xt.cpu().numpy(), et.cpu().numpy(), yt.cpu().numpy(), STD, GAMMA, MU, SIGMA), 'guidance',
           'guidance of transposed views')


# ------------------------------------------------------------------------------------------------------------ fused guidance
GUIDANCE = [
    ((3, 16, 3), (S(None, None, 4), S(0, None, 2))),                             # one leading dim
    ((3, 16, 3), (S(2, 12, 4), S(1, 3))),                                        # ... slices with stops
    ((2, 3, 16, 3), (S(None, None, 8), S(0, 1))),                                # two leading dims
    ((2, 3, 16, 3), (S(1, -2, 5), S(None, -1))),
    ((2, 3, 2, 6, 7), (S(1, None, 2), S(None, 6, 3))),                           # (B, L, C, H, W), two sliced dims
]


@pytest.mark.parametrize('shape,slices', GUIDANCE, ids=_sid)
def test_fused_guidance_formula(dev, shape, slices):
    """Each y form (A(x)'s shape, that shape without its first dim, that shape with a leading 1), mu / sigma as floats and as
    device scalars (equal bits), against A^T((y - A((x - sigma eps)/mu)) / (std^2 + gamma (sigma/mu)^2)) in float64."""
    from sda_amd import observe as Ob
    op, ref = Ob.Subsample(slices), R.subsample(shape, slices)
    o = ref.out_shape
    x, eps = _randn(shape, 40), _randn(shape, 41)
    pair = torch.tensor([MU, SIGMA], device=dev)
    for k, yshape in enumerate((o, o[1:], (1,) + o[1:])):
        y = _randn(yshape, 42 + k)
        g = op.gaussian_guidance(x.to(dev), eps.to(dev), y.to(dev), STD, GAMMA, MU, SIGMA)
        assert g is not None, yshape
        _close(g, R.gaussian_guidance(ref, x.numpy(), eps.numpy(), y.numpy(), STD, GAMMA, MU, SIGMA), 'guidance', f'y {yshape}')
        for mu_d, sg_d in ((pair[0], pair[1]),                                                      # adjacent in one buffer
                           (torch.tensor(MU, device=dev), torch.tensor(SIGMA, device=dev)), (torch.tensor(MU, device=dev), SIGMA)):
            g2 = op.gaussian_guidance(x.to(dev), eps.to(dev), y.to(dev), STD, GAMMA, mu_d, sg_d)
            assert torch.equal(g, g2), f'device mu / sigma, y {yshape}'
    # what does not broadcast over the leading axis goes to the general path
    for bad in (o[2:], (o[0],) + (1,) * (len(o) - 1), o[:1] + (1,) + o[2:], (2,) + o):
        if tuple(bad) in (o, o[1:], (1,) + o[1:]):
            continue
        assert op.gaussian_guidance(x.to(dev), eps.to(dev), torch.zeros(bad, device=dev), STD, GAMMA, MU, SIGMA) is None, bad


# -------------------------------------------------------------------------------------------------------------- edge geometry
@pytest.mark.parametrize('hw', [(3, 3), (3, 8), (5, 7), (16, 4)])
def test_edge_vorticity(dev, hw):
    from sda_amd import observe as Ob
    shape = (3, 7, 2) + hw
    ref = R.vorticity(shape)
    x, r = _randn(shape, 50), _randn(ref.out_shape, 51)
    _close(Ob.Vorticity()(x.to(dev)), ref.forward(x.numpy()), 'vorticity', f'vorticity {hw}')
    _close(Ob.Vorticity().adjoint(r.to(dev), shape), ref.adjoint(r.numpy()), 'vorticity', f'vorticity adjoint {hw}')


@pytest.mark.parametrize('plane,f', [((6, 12), 1), ((6, 12), 2), ((6, 12), 6), ((12, 4), 4), ((5, 5), 5), ((9, 15), 3)])
def test_edge_coarsen(dev, plane, f):
    from sda_amd import observe as Ob
    shape = (3, 5) + plane
    ref = R.coarsen(shape, f)
    x, r = _randn(shape, 52), _randn(ref.out_shape, 53)
    assert Ob.Coarsen(f).out_shape(shape) == ref.out_shape
    _close(Ob.Coarsen(f)(x.to(dev)), ref.forward(x.numpy()), 'coarsen', f'coarsen {plane} / {f}')
    _close(Ob.Coarsen(f).adjoint(r.to(dev), shape), ref.adjoint(r.numpy()), 'coarsen', f'coarsen adjoint {plane} / {f}')


@pytest.mark.parametrize('shape,dim,i,j', [((3, 5, 7, 11), 1, 2, 2), ((3, 5, 7, 11), -1, -2, 0), ((3, 5, 7, 11), -2, -1, -3),
                                           ((3, 5, 7, 11), 0, 2, 0), ((300,), 0, 7, -7), ((3, 5, 7, 11), -3, -5, 4)])
def test_edge_timediff(dev, shape, dim, i, j):
    from sda_amd import observe as Ob
    op, ref = Ob.TimeDiff(dim, i, j), R.timediff(shape, dim, i, j)
    x, r = _randn(shape, 54), _randn(ref.out_shape, 55)
    assert op.out_shape(shape) == ref.out_shape
    _exact(op(x.to(dev)), ref.forward(x.numpy()), 'timediff')
    g = op.adjoint(r.to(dev), shape)
    _exact(g, ref.adjoint(r.numpy()), 'timediff adjoint')
    if i % shape[dim] == j % shape[dim]:
        assert not g.any() and not op(x.to(dev)).any()


@pytest.mark.parametrize('mshape', [(11,), (7, 11), (1, 7, 11), (1, 1, 7, 11), (5, 7, 11), (1,)])
def test_edge_mask_shapes(dev, mshape):
    """Masks with fewer dims than the data's trailing block and masks with leading 1s broadcast as ``x * mask`` does."""
    from sda_amd import observe as Ob
    shape = (3, 5, 7, 11)
    m = (_randn(mshape, 56) > 0).float() * 0.75 + 0.25 * (_randn(mshape, 57) > 0).float()
    x = _randn(shape, 58)
    op = Ob.Mask(m)
    _exact(op(x.to(dev)), x.double().numpy() * m.double().numpy(), f'mask {mshape}')
    _exact(op.adjoint(x.to(dev), shape), R.mask(shape, m.numpy()).adjoint(x.numpy()), f'mask adjoint {mshape}')


def test_edge_mask_refuses_other_shapes(dev):
    from sda_amd import _lib, observe as Ob
    x = torch.zeros(3, 5, 7, 11, device=dev)
    for mshape in ((7,), (5, 1, 11), (1, 1, 1, 7, 11), (3, 5, 7, 10)):
        with pytest.raises(_lib.SdaHipError):
            Ob.Mask(torch.ones(mshape))(x)


def test_edge_mask_zero_times_nan(dev):
    """IEEE products, not a select: 0 x NaN stays NaN, 0 x (-v) is -0; the mask is zero exactly where x is finite."""
    from sda_amd import observe as Ob
    x = _randn((3, 5, 7, 11), 59)
    nan = _randn((3, 5, 7, 11), 60) > 1.0
    x[nan] = float('nan')
    out = Ob.Mask((nan).float())(x.to(dev)).cpu()
    assert torch.equal(out.isnan(), nan)
    assert not out[~nan].any() and torch.equal(out[~nan].signbit(), x[~nan].signbit())
    out = Ob.Mask(torch.zeros(7, 11))(x.to(dev)).cpu()
    assert torch.equal(out.isnan(), nan) and not out[~nan].any()


PW_EDGE = [0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 3e38, -3e38]


@pytest.mark.parametrize('kind', ['saturate', 'tanh', 'square', 'abs'])
def test_pointwise_edge_values(dev, kind):
    """Each value is judged on its own scale (one-element comparisons); what the float32-rounded reference makes infinite or
    zero must be exactly that."""
    from sda_amd import observe as Ob
    x = torch.tensor(PW_EDGE)
    r = torch.tensor([1.5, -2.0] * (len(PW_EDGE) // 2))
    out, vjp = Ob.Pointwise(kind).linearize(x.to(dev))
    got_f, got_g = out.cpu(), vjp(r.to(dev)).cpu()
    ref = R.Pointwise(x.shape, kind)
    want_f, want_vjp = ref.linearize(x.numpy())
    with np.errstate(over='ignore'):
        want_f, want_g = _t(want_f).float(), _t(want_vjp(r.numpy())).float()
    for k, v in enumerate(PW_EDGE):
        for got, want, what in ((got_f, want_f, kind), (got_g, want_g, kind + ' vjp')):
            if not torch.isfinite(want[k]) or want[k] == 0:
                assert got[k] == want[k], f'{what} at {v!r}: {got[k].item()!r} vs {want[k].item()!r}'
            else:
                _close(got[k:k + 1], want[k:k + 1].numpy(), 'pointwise', f'{what} at {v!r}')
    if kind == 'abs':
        assert torch.equal(got_f, x.abs()) and not got_f.signbit().any()
        assert torch.equal(got_g, r * torch.tensor([0.0, 0.0, 1, -1, 1, -1, 1, -1]))


# ---------------------------------------------------------------------------------------------------------- adjoint identity
@pytest.mark.parametrize('name', LINEAR_NAMES)
def test_adjoint_identity(dev, name):
    """<A x, r> = <x, A^T r> with A x and A^T r from the device and both inner products in float64 on the host."""
    shape, make, make_ref, exact, family = _linear_cases()[name]
    op = make()
    x = _randn(shape, 70)
    ax = op(x.to(dev)).cpu().double()
    r = _randn(ax.shape, 71)
    atr = op.adjoint(r.to(dev), shape).cpu().double()
    lhs, rhs = (ax * r.double()).sum().item(), (x.double() * atr).sum().item()
    scale = ((ax * ax).sum() * (r.double() * r.double()).sum()).sqrt().item()
    print(f'OBSERVE-ERR identity {name} {abs(lhs - rhs) / scale:.3e}')
    assert abs(lhs - rhs) <= TOL['identity'] * scale, f'{name}: <Ax, r> = {lhs!r}, <x, A^T r> = {rhs!r}'


# per kind: sup |f''|, sup |f'''| away from 0, and the jump of f' at 0
_PW_DERIV_BOUNDS = {'saturate': (2.0, 6.0, 0.0), 'tanh': (0.77, 2.0, 0.0), 'square': (2.0, 0.0, 0.0), 'abs': (0.0, 0.0, 2.0)}
FD_STEP = 1e-3


def _nonlinear_cases():
    from sda_amd import observe as Ob
    front = (lambda q: R.subsample(q, (S(None, None, 3), S(None), S(None), S(None))), lambda q: R.coarsen(q, 2), R.vorticity)
    crop = (S(1, 7), S(1, 7))
    cases = {kind: ((5, 7, 33), lambda kind=kind: Ob.Pointwise(kind), (), kind, ()) for kind in _PW_DERIV_BOUNDS}
    cases['cell23 saturating sensor'] = (
        (2, 9, 2, 16, 16), lambda: Ob.Compose(Ob.Subsample.frames(3), Ob.Coarsen(2), Ob.Vorticity(), Ob.Pointwise('saturate'), Ob.Crop(crop)),
        front, 'saturate', (lambda q: R.subsample(q, crop),))
    return cases


@pytest.mark.parametrize('name', NONLINEAR_NAMES)
def test_nonlinear_adjoint_identity(dev, name):
    """<D, r> = <v, J^T r> for the linearisation of a chain L2 . f . L1 (f pointwise), with J^T r from the device and
    D = (F(x + h v) - F(x - h v)) / 2h from the float64 reference, h = 1e-3.

    The bound on |<D, r> - <J v, r>| is the truncation error of the central difference.  With u = L1 x, w = L1 v and
    r' = L2^T r, <D - J v, r> = sum_k r'_k w_k (mean of f' over [u_k - h w_k, u_k + h w_k] - f'(u_k)), because
    f(u + h w) - f(u - h w) is the integral of f' over that interval.  Where the interval does not contain 0, f is C^3 on it
    and the symmetric mean differs from f'(u) by at most sup|f'''| (h w)^2 / 6.  Where it contains 0 (the kink of |.|),
    the difference is at most (jump of f' at 0) + sup|f''| h |w|.  Both are evaluated from the reference's u, w, r' alone."""
    shape, make, front, kind, back = _nonlinear_cases()[name]
    L1 = R.Chain(shape, *front)
    f = R.Pointwise(L1.out_shape, kind)
    L2 = R.Chain(f.out_shape, *back)
    F = lambda z: L2.forward(f.forward(L1.forward(z)))
    x, v = (_randn(shape, 72) * 1.5).double().numpy(), _randn(shape, 73).double().numpy()       # x, r: float32 values
    r = _randn(L2.out_shape, 74).double().numpy()
    D = (F(x + FD_STEP * v) - F(x - FD_STEP * v)) / (2 * FD_STEP)
    u, w, rp = L1.forward(x), L1.forward(v), L2.adjoint(r)
    m2, m3, jump = _PW_DERIV_BOUNDS[kind]
    straddle = np.abs(u) <= FD_STEP * np.abs(w)
    per = np.where(straddle, jump + m2 * FD_STEP * np.abs(w), m3 * (FD_STEP * w) ** 2 / 6)
    fd_bound = float((np.abs(rp) * np.abs(w) * per).sum())

    op = make()
    out, vjp = op.linearize(torch.from_numpy(x).float().to(dev))
    g = vjp(torch.from_numpy(r).float().to(dev)).cpu().double().numpy()
    lhs, rhs = float((D * r).sum()), float((v * g).sum())
    scale = float(np.sqrt((D * D).sum() * (r * r).sum()))
    print(f'OBSERVE-ERR identity {name} {max(abs(lhs - rhs) - fd_bound, 0.0) / scale:.3e} (fd bound {fd_bound / scale:.3e})')
    assert abs(lhs - rhs) <= fd_bound + TOL['identity'] * scale, f'{name}: <D, r> = {lhs!r}, <v, J^T r> = {rhs!r}, fd bound {fd_bound:.3e}'
