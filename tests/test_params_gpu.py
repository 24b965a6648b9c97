"""The parameter sweep of tests/param_cases.py on the device: tape constants -> float64 and float32 interpreters
(csrc/sdf_interp.h) -> the interval passes of the meshing path (csrc/sdf_interval.h: pruning, culling), with oblique,
reversed, degenerate, NaN, infinite and extreme parameters -- the random-tree tests of test_gpu.py stay inside comfortable
ranges.  tests/test_params_host.py holds the same cases to the recorded reference on the CPU.  All need an MI355X.

Loops of the device code whose trip count comes from data, read for NaN / inf input before any case went to a device:
  * L_POLYGON (sdf_interp.h, sdf_interval.h): the vertex count c[0], a count the lowering wrote (len(points)), never a
    parameter's value;
  * L_CIRC_PREP's sector search: c[2] rotations, written by the lowering only for pi / 4096 <= da <= pi (at most 13); a
    NaN, infinite, negative or zero da takes the polar form, which has no loop;
  * the sampled-field leaves (texture2d, grid3d: bisection over the grid's axes): no case here has one.
The libm forms (sincos64, atan2, hypot, np_mod) are straight-line code.  So no case is host-only."""
import numpy as np
import pytest

import float32_ref as fr
import oracle
import param_cases
from conftest import value_tolerance
from sdf_amd import tape
from test_float32_gpu import _held_to_the_checker
from test_gpu import _both_ways
from test_float32_gpu import float32
from test_params_host import F32_NO_ANSWER, _lowering_cases, golden_params  # noqa: F401  (golden_params: the fixture)
from test_register_slots import is_trig

pytestmark = pytest.mark.gpu

HOST_ONLY = {}          # case -> why it is not sent to a device (see the head comment: none)
CASES = [n for n in _lowering_cases() if n not in HOST_ONLY]

# 66 samples per axis over [-1.6, 1.6): two whole batches of 32 and a ragged one per axis -- the smallest grid on which
# the batch, cell-group and ragged-edge decisions of the interval passes all occur
AXIS = np.arange(66) * (3.2 / 66) - 1.6


@pytest.fixture(scope='module')
def P32():
    return fr.points()


@pytest.mark.parametrize('name', CASES)
def test_float64_values(name, ns, eng, golden_values, golden_params, oracle_lib):  # noqa: F811
    """eval_points against the checker -- the same NaN mask; bit for bit unless the tape has libm ops (test_gpu.TRIG's
    rule, read off the opcodes: test_register_slots.is_trig), then within `value_tolerance` -- and against the reference"""
    P = golden_values['P']
    f = param_cases.build(name, ns)
    v = eng.eval_points(f, P)
    o = oracle_lib.evaluate(f, P).reshape(-1)
    ref = golden_params['v_' + name]
    assert v.shape == o.shape and np.array_equal(np.isnan(v), np.isnan(o))
    if is_trig(tape.lower(f)):
        ok = ~np.isnan(o) & (v != o)
        assert np.all(np.abs(v[ok] - o[ok]) <= value_tolerance(o[ok], P[ok]))
    else:
        assert np.array_equal(v, o, equal_nan=True)
    assert np.array_equal(np.isnan(v), np.isnan(ref))
    ok = ~np.isnan(ref) & (v != ref)
    assert np.all(np.abs(v[ok] - ref[ok]) <= value_tolerance(ref[ok], P[ok]))


@pytest.mark.parametrize('name', CASES)
def test_float32_values(name, ns, eng, P32, oracle_lib):
    """the rule of test_float32_gpu.py on every case; where a constant is no float32 number and the float checker is NaN
    for it (F32_NO_ANSWER, test_params_host.py), the device's float32 values are NaN like the float checker's"""
    f = param_cases.build(name, ns)
    if name in F32_NO_ANSWER:
        with float32(eng):
            v = eng.eval_points(f, P32)
        assert np.array_equal(np.isnan(v), np.isnan(oracle_lib.evaluate_f32(f, P32).reshape(-1))), name
        return
    _held_to_the_checker(eng, f, P32, name)


@pytest.mark.parametrize('name', CASES)
def test_meshing_with_the_interval_passes_on_and_off(name, ns, eng):
    """kinds and soups with pruning and culling on, with both off, and of the checker: identical.  A tape the lowering
    marks `intervals = False` (every NAN_MODELS case) must come through the passes-on call with nothing pruned and
    nothing culled."""
    f = param_cases.build(name, ns)
    t = tape.lower(f)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, AXIS, AXIS, AXIS)
    ref = oracle.generate(f, AXIS, AXIS, AXIS, 32, True)
    assert s0['n_pruned_instrs'] == 0 and s0['n_sampled_voxels'] == s0['n_eval_voxels']
    assert np.array_equal(k1, k0) and np.array_equal(k1, ref.kinds)
    assert p1.shape == p0.shape == ref.points.shape
    assert np.array_equal(p1, p0, equal_nan=True)      # (a NaN sample next to a finite one: vertices NaN in all three coordinates, like the reference's)
    if is_trig(t):     # (the device's libm against glibc: the rule of test_gpu.py::test_interval_passes_identity_and_oracle_for_every_fixture)
        if len(p1):
            assert np.abs(p1 - ref.points).max() <= 1e-5 * 3.2 and (p1 == ref.points).mean() > 0.999
    else:
        assert np.array_equal(p1, ref.points, equal_nan=True)
    assert (name not in param_cases.NAN_MODELS) or not t.intervals
    if not t.intervals:
        assert s1['n_pruned_instrs'] == 0 and s1['n_sampled_voxels'] == s1['n_eval_voxels']


def test_the_meshing_sweep_is_not_empty(ns):
    """most cases have a surface inside the test grid (counted on the checker's soups)"""
    n = sum(len(oracle.generate(param_cases.build(name, ns), AXIS, AXIS, AXIS, 32, True).points) > 0 for name in CASES)
    assert n >= 100, n
