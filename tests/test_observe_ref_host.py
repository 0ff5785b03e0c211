"""CPU: the float64 reference of the observation operators (tests/observe_ref.py) checks itself -- its index lists against
plain array expressions, its adjoints against the inner-product identity, its dense forms (used for the tensors past the
launch-grid cap in tests/test_gpu_observe.py) against the index lists -- and the launch-free parts of sda_amd.observe
(out_shape, the 5-D fold of Subsample) against numpy's slicing."""
import numpy as np
import pytest

from tests import observe_ref as R

S = slice
rng = np.random.default_rng(5)


def _maps():
    m = (rng.standard_normal((6, 8)) > 0) * 0.5
    return [
        R.subsample((3, 5, 6, 8), (S(1, None, 2), S(None, -1, 3))),
        R.subsample((13, 11, 7), (S(-9, -2, 3), S(-6, None, 4))),
        R.select((3, 5, 2, 6, 8), -4, -2),
        R.coarsen((3, 6, 12), 6), R.coarsen((3, 6, 12), 1), R.coarsen((2, 9, 15), 3),
        R.vorticity((3, 2, 3, 3)), R.vorticity((2, 2, 5, 7)), R.vorticity((2, 2, 16, 4)),
        R.mask((3, 2, 6, 8), m), R.timediff((3, 5, 7), 1, 0, -1), R.timediff((3, 5, 7), -1, 2, 2),
        R.Chain((2, 9, 2, 6, 8), lambda q: R.select(q, -4, -1), R.vorticity, lambda q: R.mask(q, m)),
    ]


@pytest.mark.parametrize('k', range(13))
def test_reference_adjoint_is_the_transpose(k):
    A = _maps()[k]
    x, r = rng.standard_normal(A.in_shape), rng.standard_normal(A.out_shape)
    lhs, rhs = (A.forward(x) * r).sum(), (x * A.adjoint(r)).sum()
    assert abs(lhs - rhs) <= 1e-13 * np.sqrt((x * x).sum() * (r * r).sum())


def test_reference_forwards_match_plain_array_expressions():
    x = rng.standard_normal((3, 2, 6, 12))
    assert np.array_equal(R.subsample(x.shape, (S(1, None, 2), S(None, -1, 5))).forward(x), x[..., 1::2, :-1:5])
    assert np.array_equal(R.select(x.shape, -3, -1).forward(x), x[:, -1])
    assert np.allclose(R.coarsen(x.shape, 3).forward(x), x.reshape(3, 2, 2, 3, 4, 3).mean(axis=(3, 5)), rtol=0, atol=1e-15)
    u, v = x[:, 0], x[:, 1]
    vort = (np.roll(u, -1, -1) - np.roll(u, 1, -1)) / 2 - (np.roll(v, -1, -2) - np.roll(v, 1, -2)) / 2
    assert np.allclose(R.vorticity(x.shape).forward(x), vort, rtol=0, atol=1e-15)
    assert np.array_equal(R.timediff(x.shape, 2, 1, -1).forward(x), x[:, :, 1] - x[:, :, -1])
    m = rng.standard_normal((1, 12))
    assert np.array_equal(R.mask(x.shape, m).forward(x), x * m)
    for kind, f in (('saturate', lambda t: t / (1 + abs(t))), ('tanh', np.tanh), ('square', np.square), ('abs', abs)):
        p = R.Pointwise(x.shape, kind)
        out, vjp = p.linearize(x)
        assert np.array_equal(out, f(x))
        h = 1e-6
        assert np.allclose(vjp(np.ones(x.shape)), (f(x + h) - f(x - h)) / (2 * h), rtol=0, atol=1e-8)


def test_dense_forms_match_the_index_lists():
    x = rng.standard_normal((3, 4, 2, 6, 8))
    sl = (S(1, None, 2), S(None, -1, 3))
    A = R.subsample(x.shape, sl)
    r = rng.standard_normal(A.out_shape)
    assert np.array_equal(R.subsample_dense(x, sl), A.forward(x))
    assert np.array_equal(R.subsample_adjoint_dense(r, x.shape, sl), A.adjoint(r))
    A = R.coarsen(x.shape, 2)
    r = rng.standard_normal(A.out_shape)
    assert np.allclose(R.coarsen_adjoint_dense(r, 2), A.adjoint(r), rtol=0, atol=1e-15)
    A = R.vorticity(x.shape)
    r = rng.standard_normal(A.out_shape)
    assert np.allclose(R.vorticity_dense(x), A.forward(x), rtol=0, atol=1e-15)
    assert np.allclose(R.vorticity_adjoint_dense(r), A.adjoint(r), rtol=0, atol=1e-15)
    A = R.timediff(x.shape, 1, 0, -1)
    r = rng.standard_normal(A.out_shape)
    assert np.array_equal(R.timediff_dense(x, 1, 0, -1), A.forward(x))
    assert np.array_equal(R.timediff_adjoint_dense(r, x.shape, 1, 0, -1), A.adjoint(r))
    assert R.vorticity_dense(x.astype(np.float32)).dtype == np.float32
    assert R.coarsen_adjoint_dense(r.astype(np.float32)[..., :2, :2], 2).dtype == np.float32


def test_guidance_formula_of_the_reference():
    shape, sl = (3, 9, 4), (S(1, None, 4), S(None, 3))
    A = R.subsample(shape, sl)
    x, eps, y = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(A.out_shape[1:])
    g = R.gaussian_guidance(A, x, eps, y, 0.3, 0.02, 0.8, 0.6)
    want = np.zeros(shape)
    want[..., 1::4, :3] = (y - ((x - 0.6 * eps) / 0.8)[..., 1::4, :3]) / (0.3 ** 2 + 0.02 * (0.6 / 0.8) ** 2)
    assert np.allclose(g, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize('shape,slices', [
    ((13, 11, 7), (S(None, None, 3),)), ((3, 2, 13, 11, 7), (S(None, None, 2), S(7, 12, 2), S(3, 10, 4), S(None, None, 3))),
    ((2, 3, 5, 11, 7), (S(None), S(1, None, 2), S(None, None, 2), S(5, 10, 3), S(None, -1))),
    ((1, 1, 2, 3, 5, 11, 7), (S(1, None), S(None, None, 2), S(0, 4, 3), S(2, 9, 5), S(3, None, 3))),
    ((13, 11, 7), (S(-9, -2, 3), S(-6, None, 4))), ((13, 11, 7), (S(4, None, 20), S(6, None, 9))), ((7,), (S(1, None, 3),)),
    ((2, 2, 2, 13, 11, 7), (S(None, None, 4), S(1, 6, 2))), ((13, 11, 7), ())])
def test_subsample_fold_describes_the_numpy_slice(shape, slices):
    """Subsample._spec / _stop (the five size / start / step / stop entries handed to the kernels) enumerate exactly the flat
    positions numpy's slicing selects, in its order; out_shape is numpy's shape."""
    from sda_amd import observe as Ob
    op = Ob.Subsample(slices)
    size, start, step, stops = op._spec(shape)
    stop = op._stop(size, stops)
    assert len(size) == len(start) == len(step) == len(stop) == 5 and int(np.prod(size)) == int(np.prod(shape))
    picked = np.arange(int(np.prod(size))).reshape(size)[tuple(S(a, b, c) for a, b, c in zip(start, stop, step))]
    want = np.arange(int(np.prod(shape))).reshape(shape)[(Ellipsis,) + tuple(slices)]
    assert np.array_equal(picked.reshape(-1), want.reshape(-1))
    assert op.out_shape(shape) == want.shape


def test_subsample_six_dims_of_slices_are_refused():
    from sda_amd import observe as Ob
    with pytest.raises(ValueError):
        Ob.Subsample((S(None),) * 6)
    with pytest.raises(ValueError):
        Ob.Subsample((S(None),) * 5)._spec((2, 3, 4, 5, 6, 7))          # five sliced dims behind a real leading dim: six
