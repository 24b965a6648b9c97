"""What the float32 tests share (test_float32_host.py, test_float32_gpu.py): the points, the unit and the envelope.

The float32 interpreter of the product is not compared with itself: the CPU checker is built twice from one source
(oracle/sdf_oracle.c, `real` = double / float) and the distance between the two builds on a model, in units of float32
resolution, is the model's envelope E.  The device then has to stay within max(16, 4 E) units of the float64 checker.

  unit     u = 2^-24 * max(|v64|, |P|inf, 1): half a float32 ulp of a number of the size of the value or of the point it came from
           (a distance is a difference of coordinate-sized numbers), never below that of 1
  points   the rows of values.npz['P'] with |P|inf <= 16, rounded to float32 -- 596 of 600; the four dropped rows are the
           +-1e3 and +-1e9 points, where float32 has no useful answer for a twist or a sine.  Both precisions see the same input.
  floor 16 and factor 4: margin for the device's libm (ocml against glibc), a different order of summation and the polar form of
           circular_array, which float32 takes where float64 rotates.
"""
import os

import numpy as np

from conftest import GOLDEN

FLOOR = 16.0
FACTOR = 4.0

# fixtures whose float32 envelope exceeds the floor -- measured with the float build of the checker, not with the device.  All three
# are easings through bend_linear; E and the number of points (of 596) above 16 units, as test_float32_host.py prints them:
#   ease_in_out_circ  375.15   1 point   the point (0, 1e-9, 1e-9): t = 0.5 + 5e-10, where the two quarter circles meet with a vertical
#                                        tangent.  float64 gets 0.5 (sqrt(1 - v^2) + 1) with v = -1 + 1e-9, sqrt(2e-9) = 4.5e-5 above the
#                                        junction; in float32 t IS 0.5 and the root is 0.  Every other point: <= 1.9 units
#   ease_out_bounce    40.98   7 points  t in [8/11, 9/10): 4356/361 t^2 - 35442/1805 t + 16061/1805, terms of ~9 that cancel to a
#                                        value <= 1, which then moves the capsule
#   ease_in_bounce     20.18   5 points  the same curve, mirrored (1 - out_bounce(1 - t))
# (every other fixture: E <= 12.3, ease_in_out_bounce; median 2.1)
ILL_CONDITIONED = ('ease_in_bounce', 'ease_in_out_circ', 'ease_out_bounce')


def part2_points(P):
    """rows with |P|inf <= 16, rounded to float32 (returned as float64: what every entry point takes)"""
    P = np.asarray(P, dtype=np.float64)
    P = P[np.abs(P).max(axis=1) <= 16.0]
    return np.ascontiguousarray(P.astype(np.float32).astype(np.float64))


def points():
    return part2_points(np.load(os.path.join(GOLDEN, 'values.npz'))['P'])


def unit(v64, P):
    return 2.0 ** -24 * np.maximum(np.maximum(np.abs(v64), np.abs(P).max(axis=1)), 1.0)


def in_units(v, v64, P):
    """|v - v64| / u per point; NaN where either is NaN (the callers compare the NaN patterns first)"""
    return np.abs(v - v64) / unit(v64, P)


def envelope(oracle, f, P):
    """(v64, units of the float checker per point): both builds of the checker on the same model and points"""
    v64 = oracle.evaluate(f, P)
    v32 = oracle.evaluate_f32(f, P)
    assert np.array_equal(np.isnan(v32), np.isnan(v64)), 'the two builds of the checker disagree about NaN'
    return v64, in_units(v32, v64, P)


def e_max(e):
    e = e[~np.isnan(e)]
    return float(e.max()) if len(e) else 0.0


def tolerance_units(e):
    """T = max(16, 4 E)"""
    return max(FLOOR, FACTOR * e_max(e))
