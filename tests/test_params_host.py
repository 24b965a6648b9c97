"""The parameter sweep of tests/param_cases.py on the host: the front end (d2 / d3 / dn / ease -> IR), the lowering
(sdf_amd/tape.py) and the CPU checker against the recorded reference (tests/golden/values_params.npz, made by
tools/make_golden_params.py), and the host build of the interval interpreter (csrc/sdf_interval.h) against the checker.

tests/fixtures.py holds every documented function at one parameter set; here each builder also gets oblique, reversed,
degenerate, NaN, infinite and extreme parameters -- among them the models that are NaN at every point, for which an
interval run must not come back with a finite interval (param_cases.NAN_MODELS)."""
import builtins
import os
import re
import zlib

import numpy as np
import pytest

import param_cases
from conftest import GOLDEN, value_tolerance
from test_interval_host import _check_tape_enclosure, tape_lib  # noqa: F401  (tape_lib: the fixture)

# what the reference accepts and this implementation refuses on purpose: name -> exception type.  A Python callable as
# an easing cannot be lowered to the tape (sdf_amd/ease.py easing_id): ease.Easing objects only.
REFUSED_BY_DESIGN = {
    'ease_lambda': 'OpaqueSDFError',
}

# GENERIC cases left out of the "small boxes get finite intervals" assertion: ONLY those whose reference values are NaN
# at more than 10 % of the shared points (test_generic_cases_left_out_of_tightness_are_nan_in_the_reference)
NOT_TIGHT = []

# cases with a constant that is no float32 number (1e300 becomes inf) AND whose float32 value is NaN for it where the
# float64 value is not: the two builds of the checker disagree about NaN, so the float32 rule of float32_ref.py (which
# starts from their agreement) has no answer; test_params_gpu.py holds the device to the float32 checker's NaN there
F32_NO_ANSWER = ['repeat_huge_spacing', 'twist_huge']


@pytest.fixture(scope='module')
def golden_params():
    return np.load(os.path.join(GOLDEN, 'values_params.npz'))


def _exception_class(name):
    from sdf_amd import ir
    return getattr(ir, name, None) or getattr(builtins, name)


def _expected_error(name, golden_params):
    """the exception class this case must raise, or None"""
    if 'e_' + name in golden_params.files:
        assert name not in REFUSED_BY_DESIGN
        return _exception_class(str(golden_params['e_' + name]))
    if name in REFUSED_BY_DESIGN:
        return _exception_class(REFUSED_BY_DESIGN[name])
    return None


def _lowers(name, golden_params):
    return 'e_' + name not in golden_params.files and name not in REFUSED_BY_DESIGN


def _lowering_cases():
    """the cases neither the reference nor this implementation refuses"""
    g = np.load(os.path.join(GOLDEN, 'values_params.npz'))
    return sorted(n for n in param_cases.CASES if _lowers(n, g))


def test_table_and_golden_agree(golden_params):
    """one record per case, nothing else; every refusal by design is a case the reference evaluates"""
    assert sorted(k[2:] for k in golden_params.files if k[:2] in ('v_', 'e_')) == sorted(param_cases.CASES)
    assert 150 <= len(param_cases.CASES) <= 250
    assert all('v_' + n in golden_params.files for n in REFUSED_BY_DESIGN)
    assert os.path.getsize(os.path.join(GOLDEN, 'values_params.npz')) < os.path.getsize(os.path.join(GOLDEN, 'values.npz'))


def test_every_public_builder_is_swept():
    """every builder and method of d2 / d3 / dn (the names of test_host.py::test_public_names_cover_reference_surface)
    is called by a case of each class that applies to it: at least by one generic case"""
    builders = '''
    sphere plane slab box rounded_box wireframe_box torus capsule cylinder capped_cylinder
    rounded_cylinder capped_cone rounded_cone ellipsoid pyramid tetrahedron octahedron
    dodecahedron icosahedron
    translate scale rotate rotate_to orient circular_array elongate twist bend bend_linear
    bend_radial transition_linear transition_radial wrap_around slice
    union difference intersection blend negate dilate erode shell repeat
    circle line rectangle rounded_rectangle equilateral_triangle hexagon rounded_x polygon vesica
    extrude extrude_to revolve
    '''.split()
    text = '\n'.join(param_cases.GENERIC.values())
    operators = {'union': r'\|', 'difference': r' - ', 'intersection': r'&'}
    missing = [b for b in builders
               if not re.search(r'(?<![A-Za-z_])%s\(' % b, text) and not (b in operators and re.search(operators[b], text))]
    assert not missing, missing


@pytest.mark.parametrize('name', sorted(param_cases.CASES))
def test_checker_matches_the_reference(name, ns, golden_params, golden_values, oracle_lib):
    """front end -> IR -> CPU checker against the recorded reference values: the same NaN mask, values within
    `value_tolerance`; where the reference raises, the same exception class here (from the builder, the lowering or the
    evaluation, wherever it surfaces)"""
    from sdf_amd import tape
    P = golden_values['P']
    err = _expected_error(name, golden_params)
    if err is not None:
        with pytest.raises(err) as info:
            f = param_cases.build(name, ns)
            tape.lower(f)
            oracle_lib.evaluate(f, P)
        assert type(info.value) is err, type(info.value)
        return
    f = param_cases.build(name, ns)
    tape.lower(f)
    v = oracle_lib.evaluate(f, P).reshape(-1)
    r = golden_params['v_' + name]
    assert np.array_equal(np.isnan(v), np.isnan(r)), (name, int(np.isnan(v).sum()), int(np.isnan(r).sum()))
    ok = ~np.isnan(r)
    same = v[ok] == r[ok]                                    # (infinities)
    d = np.abs(v[ok][~same] - r[ok][~same])
    tol = value_tolerance(r[ok], P[ok])[~same]
    assert np.all(d <= tol), (name, float(np.max(d / tol)))


@pytest.mark.parametrize('name', _lowering_cases())
def test_interval_run_encloses_the_checker(name, tape_lib, ns, golden_params, golden_values, oracle_lib):  # noqa: F811
    """the interval run of every case's tape over boxes around the shared points encloses the checker's values in them; a
    NaN value only where the interval is the whole line -- param_cases.NAN_MODELS included, whose tapes the lowering marks
    so that no interval pass runs.  Generic cases: the small boxes get finite intervals (the check is not vacuous)."""
    f = param_cases.build(name, ns)
    tight = name in param_cases.GENERIC and name not in NOT_TIGHT
    _check_tape_enclosure(name, f, tape_lib, oracle_lib, golden_values['P'], zlib.crc32(name.encode()), tight=tight)


def test_generic_cases_left_out_of_tightness_are_nan_in_the_reference(golden_params):
    for name in NOT_TIGHT:
        assert name in param_cases.GENERIC and np.isnan(golden_params['v_' + name]).mean() > 0.1, name


@pytest.mark.parametrize('name', param_cases.NAN_MODELS)
def test_nan_models_get_no_interval_pass(name, ns, golden_params):
    """every value of these is NaN in the reference; their tapes carry no operand ranges and say `intervals = False`, which
    the engine hands to the library (sdf_tape_set_intervals): neither the pruning nor the culling pass runs for them"""
    from sdf_amd import tape
    assert np.isnan(golden_params['v_' + name]).all()
    t = tape.lower(param_cases.build(name, ns))
    assert t.intervals is False and t.rstart is None and t.lstart is None


def test_well_formed_models_keep_their_interval_passes(ns, golden_params):
    """the lowering rule moves nothing for a model without NaN / infinite constants and zero divisors: every generic case
    that lowers, every fixture and every slot fixture keeps its operand ranges"""
    import fixtures
    from sdf_amd import tape
    for name in param_cases.GENERIC:
        if _lowers(name, golden_params):
            t = tape.lower(param_cases.build(name, ns))
            assert t.intervals and t.rstart is not None, name
    for name in list(fixtures.FIXTURES) + list(fixtures.SLOT_FIXTURES):
        t = tape.lower(fixtures.build(name, ns))
        assert t.intervals and (t.rstart is not None or t.n_instr > tape.PRUNE_MAX_INSTR), name


def test_float32_checker_agrees_about_nan_except_where_listed(ns, oracle_lib):
    """the premise of the float32 device test: the float and the double build of the checker have the same NaN mask on
    every case but F32_NO_ANSWER, where the float build is NaN everywhere and the double build nowhere"""
    import float32_ref as fr
    P = fr.points()
    for name in _lowering_cases():
        f = param_cases.build(name, ns)
        n64, n32 = np.isnan(oracle_lib.evaluate(f, P)), np.isnan(oracle_lib.evaluate_f32(f, P))
        if name in F32_NO_ANSWER:
            assert n32.all() and not n64.any(), name
        else:
            assert np.array_equal(n32, n64), name


def test_checker_marches_a_volume_with_nan_like_the_reference(ns, golden_params, oracle_lib):
    """extrude_to(.., 0) is positive everywhere but NaN on the plane z = 0.  The reference's `generate` (recorded) marches
    such a batch -- volume.min() is NaN, so skimage's range check passes; a NaN sample counts as inside -- and returns
    triangles of NaN.  The checker's `generate` must classify the batch and count its triangles the same way (it used
    to take the minimum over the other samples and call the batch empty, while the device meshed it).  skimage
    interpolates all three coordinates of a vertex with the NaN weight: the whole vertex is NaN, and so is the checker's
    (it used to be NaN in the coordinate along the cell edge alone; tests/test_mc_edges_host.py has more of this)."""
    from sdf_amd import core
    name = 'extrude_to_zero'
    bounds = tuple(map(tuple, golden_params['g_%s_bounds' % name]))
    X, Y, Z, _ = core.grid_axes(bounds, float(golden_params['g_%s_step' % name]))
    r = oracle_lib.generate(param_cases.build(name, ns), X, Y, Z, 32, True)
    want = golden_params['g_%s_points' % name]
    assert len(want) > 0 and np.isnan(want).all()
    assert np.array_equal(r.kinds, golden_params['g_%s_kinds' % name])
    assert r.points.shape == want.shape and np.isnan(r.points).all()
