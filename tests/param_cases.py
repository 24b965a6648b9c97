"""Parameter sweep of every public builder and method of d2 / d3 / dn / ease: the same model programs run against the
unmodified reference (tools/make_golden_params.py -> tests/golden/values_params.npz) and against the implementation
under test (tests/test_params_host.py, tests/test_params_gpu.py).

tests/fixtures.py pins each documented function at ONE parameter set; this table walks the parameter space around it:

  GENERIC      oblique / off-centre / non-unit vectors, reversed ranges, radii past the half-size, unusual counts, booleans
               of three and more children with mixed k, easing arguments in every position
  DEGENERATE   zero sizes / radii / heights, coinciding end points, zero vectors, degenerate polygons, k <= 0
  OPAQUE_EASINGS  easing curves that have no interval form, and a Python callable as an easing
  NONFINITE    NaN / inf / huge / tiny parameters in every position of a boolean

NAN_MODELS names the models whose every value is NaN although a finite sibling or a later clip / max would hide it from
an interval run (they are in the tables above under these names).

Every entry is a small program over the ``from sdf import *`` namespace that leaves the model in ``f`` -- or raises:
the recorded golden then holds the exception's class name.  This file is data, it must stay importable under Python 3.9
and must not import sdf_amd.
"""

_DUP = "[(0, 0), (1, 0), (1, 0), (1, 1), (0, 1)]"

GENERIC = {
    # --- 3-D leaves
    'sphere_off': "f = sphere(0.8, (0.3, -0.4, 0.5))",
    'plane_oblique': "f = sphere(1.5) & plane((1, -2, 0.5), (0.2, 0.1, -0.3))",
    'slab_six': "f = sphere(2) & slab(x0=-1, x1=0.5, y0=-0.7, y1=1.2, z0=-0.3, z1=0.9)",
    'slab_reversed': "f = sphere(2) & slab(z0=0.5, z1=-0.5)",
    'box_off': "f = box((0.7, 1.3, 2.1), (0.4, -0.2, 0.1))",
    'rounded_box_big_r': "f = rounded_box((1, 2, 3), 0.8)",
    'wireframe_thick': "f = wireframe_box((1, 2, 3), 0.7)",
    'torus_fat': "f = torus(0.3, 0.5)",
    'capsule_oblique': "f = capsule((-0.5, 0.2, -1), (0.7, -0.3, 0.9), 0.35)",
    'capped_cylinder_oblique': "f = capped_cylinder((-0.5, 0.2, -1), (0.7, -0.3, 0.9), 0.35)",
    'rounded_cylinder_rb_big': "f = rounded_cylinder(0.5, 0.7, 1)",
    'capped_cone_ra_lt_rb': "f = capped_cone(-Z, Z, 0.3, 0.9)",
    'capped_cone_ra_eq_rb': "f = capped_cone(-Z, Z, 0.5, 0.5)",
    # (an oblique cone by rotation: with oblique end points the reference's sqrt(papa - paba * paba * baba) turns the one
    # ulp by which np.dot of a row and of the matrix differ -- BLAS, on one machine -- into hundreds of ulp near the axis,
    # so that model has no golden a test could hold to `value_tolerance`)
    'capped_cone_oblique': "f = capped_cone(-Z, Z, 0.6, 0.1).rotate(0.9, (1, 2, 3)).translate((0.1, -0.1, 0.65))",
    'rounded_cone_r1_lt_r2': "f = rounded_cone(0.25, 0.75, 2)",
    'rounded_cone_r1_eq_r2': "f = rounded_cone(0.5, 0.5, 1.5)",
    'ellipsoid_flat': "f = ellipsoid((0.5, 1.5, 0.05))",
    'pyramid_tall': "f = pyramid(2.5)",
    'tetrahedron_dodecahedron': "f = tetrahedron(0.6).translate((0.9, -0.1, 0.3)) | dodecahedron(0.5).translate((-0.9, 0, 0))",
    'octahedron_small': "f = octahedron(0.6).rotate(0.4, (1, 1, 0))",
    'icosahedron_small': "f = icosahedron(0.45).scale((1, 2, 0.5))",
    # --- positioning
    'scale_aniso': "f = torus(1, 0.25).scale((0.5, 3, 1.25))",
    'rotate_reversed': "f = capped_cylinder(-Z, Z, 0.5).rotate(-7.5, Y)",
    'rotate_non_unit_axis': "f = box((1, 2, 3)).rotate(2.2, (1, 2, 3))",
    'rotate_to_oblique': "f = box((1, 2, 3)).rotate_to((3, -1, 2), (0.1, 0.2, -5))",
    'rotate_to_same': "f = box((1, 2, 3)).rotate_to((0, 2, 0), (0, 5, 0))",
    'orient_down': "f = capped_cone(-Z, Z, 1, 0.5).orient(-Z)",
    'circular_array_1': "f = box(0.5).circular_array(1, 1)",
    'circular_array_2': "f = box(0.5).circular_array(2, 1)",
    'circular_array_97': "f = sphere(0.1).circular_array(97, 3)",
    # --- alterations
    'elongate_mixed': "f = torus(1, 0.25).elongate((0.3, 0, 1.2))",
    'twist_reversed': "f = box((1, 2, 0.5)).twist(-3)",
    'bend_reversed': "f = box((3, 0.5, 0.5)).bend(-0.7)",
    'bend_linear_oblique': "f = capsule(-Z * 2, Z * 2, 0.25).bend_linear((0.1, 0.2, -1.5), (-0.2, 0.3, 0.7), (1, -0.5, 0.25))",
    'bend_radial_reversed': "f = box((5, 5, 0.25)).bend_radial(2, 1, -1, ease.in_out_quad)",
    'transition_linear_oblique': "f = box().transition_linear(sphere(), (0.5, -0.5, -1), (-0.5, 0.25, 1.5), ease.in_out_cubic)",
    'transition_radial_ease': "f = box().transition_radial(sphere(), 0.25, 1.5, e=ease.out_quart)",
    'transition_radial_reversed': "f = box().transition_radial(sphere(), 1.5, 0.25)",
    'wrap_around_reversed': "f = box((6, 0.5, 0.5)).orient(Y).wrap_around(3, -3)",
    'wrap_around_ease': "f = box((6, 0.5, 0.5)).orient(Y).wrap_around(-3, 3, e=ease.in_out_quad)",
    'slice_torus': "f = torus(1, 0.25).rotate(0.5, X).translate((0, 0, 0.1)).slice().extrude(0.2)",
    # --- booleans
    'union3_mixed_k': "f = union(box(1), sphere(0.7).translate((0.5, 0, 0)).k(0.2), torus(1, 0.2), capsule(-X, X, 0.3).k(0.05))",
    'difference3_mixed_k': "f = difference(box(2), sphere(1.2), cylinder(0.4).k(0.15), capsule(-X * 2, X * 2, 0.3))",
    'intersection3_mixed_k': "f = intersection(box(2), sphere(1.3).k(0.1), cylinder(1.1), plane((1, 1, 1)).k(0.3))",
    'k_before_transform': "f = box(1) | sphere(0.7).k(0.2).translate((0.5, 0, 0))",
    'k_after_transform': "f = box(1) | sphere(0.7).translate((0.5, 0, 0)).k(0.2)",
    'k_larger_than_shapes': "f = box(1) | sphere(0.7).translate((0.5, 0, 0)).k(5)",
    'blend_one': "f = sphere().blend(box(), k=1)",
    'blend_past_one': "f = sphere().blend(box(), k=1.7)",
    'dilate_negative': "f = box(1).dilate(-0.2)",
    'erode_negate': "f = box(1).erode(-0.2).negate() & sphere(2)",
    'shell_thick': "f = sphere().shell(2.5)",
    'repeat_count_only': "f = sphere(0.4).repeat(1, 2)",
    'repeat_scalar_padding': "f = sphere(0.7).repeat(1.2, padding=1)",
    'repeat_zero_spacing_axis': "f = box(0.8).repeat((1.5, 0, 0), padding=1)",
    # --- 2-D leaves and operators through extrude / revolve
    'circle_off': "f = circle(0.6, (-0.7, 0.4)).extrude(0.3)",
    'line_oblique': "f = (circle(1.5) & line((-3, 0.5), (0.2, -0.4))).extrude(0.5)",
    'slab2_reversed': "f = (circle(1) & d2.slab(x0=0.5, x1=-0.5)).extrude(0.5)",
    'rounded_rectangle_scalar': "f = rounded_rectangle((2, 1), 0.3).extrude(0.5)",
    'rounded_rectangle_big_r': "f = rounded_rectangle(np.array((2, 1)), (0.9, 0.2, 0.7, 0.4), (0.1, 0.2)).extrude(0.5)",
    'equilateral_triangle_scaled': "f = equilateral_triangle().scale(1.7).rotate(0.5).extrude(0.5)",
    'rounded_x_r_past_w': "f = rounded_x(0.2, 0.5).extrude(0.5)",
    'polygon_clockwise': "f = polygon([(0, 1.5), (1, 0.4), (2, 1), (2, 0), (0, 0)]).extrude(0.5)",
    'polygon_self_crossing': "f = polygon([(0, 0), (2, 1), (2, 0), (0, 1)]).extrude(0.5)",
    'vesica_near_r': "f = vesica(1, 0.9).extrude(0.5)",
    'translate2_rotate2': "f = rectangle((1, 0.5)).rotate(-2.5).translate((-0.4, 0.7)).extrude(0.5)",
    'scale2_aniso': "f = hexagon(0.5).scale((0.4, 2.5)).extrude(0.5)",
    'circular_array2_1': "f = rectangle((1, 0.2)).translate((1, 0)).circular_array(1).extrude(0.3)",
    'elongate2_one_axis': "f = circle(0.5).elongate((0, 0.75)).extrude(0.3)",
    'repeat2_count_only': "f = circle(0.3).repeat(1, 1).extrude(0.3)",
    'extrude_to_default_ease': "f = rectangle(2).extrude_to(circle(1), 2)",
    'revolve_zero_offset': "f = hexagon(0.5).revolve()",
    'revolve_negative_offset': "f = circle(0.4).revolve(-1.5)",
}

# easing curves without an interval form (not monotone, or through libm: csrc/sdf_interval.h ease_value) in the argument
# positions that fixtures.py does not reach; the interval run of these is the whole line by design
OPAQUE_EASINGS = {
    'ease_expo_bend': "f = capsule(-Z * 2, Z * 2, 0.25).bend_linear(-Z, Z, X * 1e3, ease.in_expo)",
    'ease_elastic_transition': "f = box().transition_linear(sphere(), -Z * 3, Z * 3, ease.in_out_elastic)",
    'ease_back_wrap': "f = box((6, 0.5, 0.5)).orient(Y).wrap_around(-3, 3, e=ease.in_back)",
    'ease_bounce_bend_radial': "f = box((5, 5, 0.25)).bend_radial(1, 2, -1, ease.out_bounce)",
    'ease_sine_extrude_to': "f = rectangle(2).extrude_to(circle(1), 2, ease.in_out_sine)",
    'ease_lambda': "f = box().transition_linear(sphere(), e=lambda t: t * t)",
}

DEGENERATE = {
    'sphere_zero': "f = sphere(0)",
    'box_zero': "f = box(0)",
    'box_negative': "f = box((-1, 1, 1))",
    'torus_zero': "f = torus(0, 0.5)",
    'rounded_cylinder_h0': "f = rounded_cylinder(0.5, 0.1, 0)",
    'rounded_cone_steep': "f = rounded_cone(0.9, 0.1, 0.5)",
    'rounded_cone_h0': "f = rounded_cone(0.5, 0.25, 0)",
    'ellipsoid_zero': "f = ellipsoid((1, 0, 1))",
    'pyramid_zero': "f = pyramid(0)",
    'capsule_same_ends': "f = capsule((.1, .2, .3), (.1, .2, .3), .4)",
    'capsule_same_ends_union': "f = capsule(Z, Z, .5) | sphere(.5)",
    'capsule_same_ends_difference': "f = sphere(1) - capsule(Z, Z, .5)",
    'capped_cylinder_same_ends': "f = capped_cylinder(Z, Z, 0.5)",
    'capped_cylinder_same_ends_union': "f = capped_cylinder(Z, Z, .5) | sphere(.5)",
    'capped_cone_same_ends_union': "f = capped_cone(Z, Z, .5, .2) | sphere(.5)",
    'bend_linear_same_ends': "f = capsule(-Z * 2, Z * 2, .25).bend_linear(Z, Z, X)",
    'transition_linear_same_ends': "f = box().transition_linear(sphere(), Z, Z)",
    'bend_radial_same_radii': "f = box((5, 5, 0.25)).bend_radial(1, 1, -1)",
    'transition_radial_same_radii': "f = box().transition_radial(sphere(), 0.5, 0.5)",
    'wrap_around_same_ends': "f = box((6, 0.5, 0.5)).orient(Y).wrap_around(1, 1)",
    'plane_zero_normal': "f = sphere() & plane((0, 0, 0))",
    'line_zero_normal': "f = (circle(1) & line((0, 0))).extrude(.5)",
    'rotate_zero_axis': "f = box((1, 2, 3)).rotate(1.0, (0, 0, 0))",
    'orient_zero': "f = box((1, 2, 3)).orient((0, 0, 0))",
    'rotate_to_zero': "f = box((1, 2, 3)).rotate_to((0, 0, 0), Z)",
    'polygon_duplicate_vertex': "f = polygon(%s).extrude(.5)" % _DUP,
    'polygon_duplicate_vertex_union': "f = polygon(%s).extrude(.5) | sphere(.3).translate((2, 0, 0))" % _DUP,
    'polygon_collinear': "f = polygon([(0, 0), (1, 0), (2, 0), (2, 1), (0, 1)]).extrude(0.5)",
    'polygon_two_vertices': "f = polygon([(0, 0), (1, 1)]).extrude(0.5)",
    'union_k_zero': "f = sphere(1) | sphere(1).k(0)",
    'union_k_zero_apart': "f = box((3, 3, 0.5)) | sphere().k(0)",
    'union_k_negative': "f = box((3, 3, 0.5)) | sphere().k(-0.25)",
    'difference_k_zero': "f = box((3, 3, 0.5)) - sphere().k(0)",
    'difference_k_negative': "f = box((3, 3, 0.5)) - sphere().k(-0.25)",
    'intersection_k_zero': "f = box((3, 3, 0.5)) & sphere().k(0)",
    'intersection_k_negative': "f = box((3, 3, 0.5)) & sphere().k(-0.25)",
    'blend_zero': "f = sphere().blend(box(), k=0)",
    'scale_zero_component': "f = sphere().scale((1, 0, 1))",
    'scale_zero_union': "f = box(1).scale(0) | sphere(.5).translate((1, 0, 0))",
    'scale_negative_component': "f = sphere().scale((1, -2, 3))",
    'scale2_zero': "f = circle(1).scale((0, 1)).extrude(0.5)",
    'vesica_d_past_r': "f = vesica(0.4, 1).extrude(0.5)",
    'rounded_rectangle_negative_r': "f = rounded_rectangle(np.array((2, 1)), (-0.1, 0.2, 0.3, 0.4)).extrude(0.5)",
    'hexagon_zero': "f = hexagon(0).extrude(0.5)",
    'shell_zero': "f = sphere().shell(0)",
    'extrude_zero': "f = hexagon(1).extrude(0)",
    'extrude_to_zero': "f = rectangle(2).extrude_to(circle(1), 0)",
    'elongate_negative': "f = torus(1, 0.25).elongate((-0.2, 0.1, 0))",
    'circular_array_zero': "f = box(0.5).translate((1, 0, 0)).circular_array(0)",
    'circular_array_negative': "f = box(0.5).circular_array(-3, 1)",
    'circular_array2_zero': "f = circle(0.2).translate((1, 0)).circular_array(0).extrude(0.3)",
    'repeat_zero_spacing': "f = sphere(0.4).repeat(0)",
}

NONFINITE = {
    # a NaN or inf parameter in the first, middle and last child of each boolean
    'nan_union_first': "f = sphere(np.nan) | box(1)",
    'nan_union_last_translate': "f = box(1).translate((np.nan, 0, 0)) | sphere(1)",
    'nan_union3_first': "f = sphere(np.nan) | box(1) | sphere(.7).translate((1, 0, 0))",
    'nan_union3_middle': "f = box(1) | sphere(np.nan) | sphere(.7).translate((1, 0, 0))",
    'nan_union3_last': "f = box(1) | sphere(.7).translate((1, 0, 0)) | sphere(np.nan)",
    'nan_intersection_first': "f = sphere(np.nan) & box(1)",
    'nan_intersection3_middle': "f = intersection(box(1), sphere(np.nan), sphere(1.2))",
    'nan_intersection3_last': "f = intersection(box(1), sphere(1.2), box((np.nan, 1, 1)))",
    'nan_difference_last': "f = box(1) - sphere(np.nan)",
    'nan_difference_first': "f = sphere(np.nan) - box(1)",
    'nan_difference3_middle': "f = difference(box(2), torus(np.nan, 0.2), sphere(0.5))",
    'nan_smooth_union_last': "f = box(1) | sphere(np.nan).k(0.2)",
    'nan_smooth_union_first': "f = sphere(np.nan) | box(1).k(0.2)",
    'nan_smooth_union3_middle': "f = union(box(1), sphere(np.nan), sphere(.7).translate((1, 0, 0)), k=0.2)",
    'nan_k': "f = box(1) | sphere(0.7).translate((0.5, 0, 0)).k(np.nan)",
    'inf_union_first': "f = sphere(np.inf) | box(1)",
    'inf_union3_middle': "f = box(1) | sphere().translate((np.inf, 0, 0)) | sphere(.7).translate((1, 0, 0))",
    'inf_intersection_last': "f = sphere(2) & box((1, np.inf, 1))",
    'inf_difference_last': "f = box(1) - cylinder(np.inf)",
    'inf_smooth_union_last': "f = box(1) | sphere(np.inf).k(0.2)",
    # extreme magnitudes
    'translate_huge': "f = sphere().translate((1e300, 0, 0)) | box(1)",
    'scale_huge': "f = sphere().scale(1e200) & box(1)",
    'sphere_tiny': "f = sphere(1e-300) | box(1e-200)",
    'dilate_inf': "f = box(1).dilate(np.inf) & sphere(1)",
    'twist_inf': "f = box().twist(np.inf)",
    'twist_huge': "f = box().twist(1e300)",
    'bend_nan': "f = box().bend(np.nan)",
    'box_inf_side': "f = box((1, np.inf, 1))",
    'rotate_inf_angle': "f = box((1, 2, 3)).rotate(np.inf, X) | sphere(0.5)",
    'repeat_huge_spacing': "f = sphere(0.5).repeat(1e300)",
    'circle_nan_extrude': "f = circle(np.nan).extrude(0.5) | sphere(0.5)",
    'k_huge': "f = box(1) | sphere(0.7).translate((0.5, 0, 0)).k(1e300)",
}

CASES = {}
for _t in (GENERIC, OPAQUE_EASINGS, DEGENERATE, NONFINITE):
    assert not set(_t) & set(CASES)
    CASES.update(_t)

# every value of these is NaN in the reference; before the lowering rule (sdf_amd/tape.py `intervals`) the interval run
# gave each of them a finite interval
NAN_MODELS = [
    'capsule_same_ends', 'polygon_duplicate_vertex', 'scale_zero_component', 'scale_zero_union',
    'transition_linear_same_ends', 'bend_linear_same_ends', 'capped_cylinder_same_ends_union', 'capsule_same_ends_union',
    'capsule_same_ends_difference', 'capped_cone_same_ends_union', 'line_zero_normal', 'plane_zero_normal',
    'rotate_zero_axis', 'orient_zero', 'rotate_to_zero', 'polygon_duplicate_vertex_union',
    'nan_union_first', 'nan_union_last_translate', 'nan_intersection_first', 'nan_difference_last',
    'nan_union3_first', 'nan_union3_middle', 'twist_inf',
]
assert len(NAN_MODELS) == 23 and all(n in CASES for n in NAN_MODELS)


def build(name, namespace):
    """exec the case's program in a copy of `namespace` and return its ``f`` (or let its exception through)"""
    ns = dict(namespace)
    exec(CASES[name], ns)
    return ns['f']
