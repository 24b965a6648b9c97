"""The float32 build of the CPU checker (oracle/libsdf_oracle_f32.so) against the float64 build, on every fixture, without a GPU.
This pins the envelope that test_float32_gpu.py takes its tolerance from (float32_ref.py says what the unit and the points are):
were the float build to drift -- a literal left in double, a libm call through the wrong width, a parameter read from the wrong
element -- the bound the device is held to would drift with it, and this is where that shows."""
import numpy as np
import pytest

import fixtures
import float32_ref as fr
import oracle

ALL = sorted(fixtures.FIXTURES) + sorted(fixtures.SLOT_FIXTURES)

# the caps on the exception list: at most 4 fixtures, each with at most 2 % of its points above the floor
MAX_EXCEPTIONS = 4
MAX_FRACTION_ABOVE = 0.02


@pytest.fixture(scope='module')
def P():
    return fr.points()


def test_the_points_are_the_596_rows_within_16_rounded_to_float32(P):
    assert P.shape == (596, 3) and P.dtype == np.float64
    assert np.array_equal(P, P.astype(np.float32).astype(np.float64)) and np.abs(P).max() <= 16.0


def test_the_exception_list_is_short_and_names_fixtures():
    assert len(fr.ILL_CONDITIONED) <= MAX_EXCEPTIONS and set(fr.ILL_CONDITIONED) <= set(ALL)


@pytest.mark.parametrize('name', ALL)
def test_float_checker_stays_within_the_envelope_of_the_float64_checker(name, ns, P):
    f = fixtures.build(name, ns)
    v64 = oracle.evaluate(f, P)
    v32 = oracle.evaluate_f32(f, P)
    assert np.array_equal(v32, v32.astype(np.float32).astype(np.float64), equal_nan=True)     # float32 values, widened
    assert np.array_equal(np.isnan(v32), np.isnan(v64))
    e = fr.in_units(v32, v64, P)
    e = e[~np.isnan(e)]
    above = int((e > fr.FLOOR).sum())
    print('%s: E = %.2f units, %d of %d points above %g' % (name, e.max(), above, len(e), fr.FLOOR))
    if name in fr.ILL_CONDITIONED:
        assert above <= MAX_FRACTION_ABOVE * len(e), (name, above)
        assert e.max() > fr.FLOOR, '%s is listed as ill-conditioned but stays within the floor: take it off the list' % name
    else:
        assert e.max() <= fr.FLOOR, (name, float(e.max()))


def test_float_checker_is_really_float32_on_the_canonical_example(ns, P):
    """ex_example is sphere(1) & box(1.5) minus three cylinders of radius 0.5 along the axes: the float build of the checker against
    NumPy float32 arithmetic on the same formulas, within 2 units -- a build that computed in double and rounded at the end would
    pass this too, but it would sit within HALF a unit of the float64 checker everywhere, and it does not (last assertion)"""
    p = P.astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    q = np.abs(p) - np.float32(0.75)
    body = np.maximum(np.sqrt((x * x + y * y) + z * z) - np.float32(1),
                      np.sqrt((np.maximum(q, 0) ** 2).sum(axis=1)) + np.minimum(q.max(axis=1), 0))
    holes = np.minimum(np.minimum(np.sqrt(y * y + z * z), np.sqrt(x * x + z * z)), np.sqrt(x * x + y * y)) - np.float32(0.5)
    want = np.maximum(body, -holes)
    assert want.dtype == np.float32
    f = fixtures.build('ex_example', ns)
    v32 = oracle.evaluate_f32(f, P)
    v64 = oracle.evaluate(f, P)
    assert np.all(np.abs(v32 - want.astype(np.float64)) <= 2.0 * fr.unit(v64, P))
    rounded = v64.astype(np.float32).astype(np.float64)
    assert np.all(fr.in_units(rounded, v64, P) <= 1.0) and (v32 != rounded).mean() > 0.1
