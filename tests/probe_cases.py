"""The cases, inputs and parameters of the probe sweep (tests/test_probe_sweep_host.py on the CPU checker,
tests/test_probe_sweep_gpu.py on the device): every model the suite knows, sent through the six kernels that inline their own
copy of the tape interpreter -- k_render, k_vertex_normals, k_vertex_thickness, k_support_rays, k_triangle_deviation,
k_vertex_snap -- with one small input per model.  The unit tests of those kernels (test_render_gpu.py, test_export_gpu.py,
test_thickness_gpu.py, test_supports_gpu.py, test_deviation_gpu.py) walk the kernels' own states on a handful of models; this
table walks the OPCODES through the kernels.

CASES: every name of fixtures.FIXTURES and fixtures.SLOT_FIXTURES, every name of param_cases.CASES whose program builds and
whose model evaluates (RAISES lists the others with the exception's class), and six sampled-leaf models: the three pictures of
tools/make_golden_texture.py extruded (L_TEXTURE2D) and the three voxel grids of tools/make_golden_custom.py (L_GRID3D; axis
lengths 31/31/15, 36/26/31 and 9/8/7: the bisection of grid3d_lookup has lane-dependent depths).  A case is swept only where its
tape has no closures (`swept`): closures take the definition on the host.  EXTRA holds the cases made for one state.

INPUT per case (`inputs`, made on the CPU, deterministic): the checker's mesh of the model on a 24^3 grid, its all-finite
triangles strided down to at most 300, plus 33 random triangles off the surface (so THIN, OPEN and miss states occur, and a
model with no surface on the grid still gets work); the welded points are np.unique of the soup's vertices: 99 .. 999 of them,
a partial last wave and several workgroups.  This module is plain data and NumPy: importable without a device."""
import math
import os

import numpy as np

import deviation_ref
import fixtures
import normals_ref
import overhang_ref
import param_cases
import render_ref
import supports_ref
import thickness_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# param_cases.CASES that raise, in the builder or at the first evaluation: name -> the exception's class name (an attribute of
# sdf_amd.ir, else a builtin).  test_params_host.py holds the first five to the recorded reference, which raises the same.
RAISES = {
    'blend_zero': 'TypeError',
    'circular_array2_zero': 'TypeError',
    'circular_array_zero': 'ZeroDivisionError',
    'ease_lambda': 'OpaqueSDFError',
    'rounded_cone_h0': 'ZeroDivisionError',
    'rounded_rectangle_scalar': 'TypeError',
}

PICTURES = ('frame', 'blobs', 'noise')
GRIDS = ('torus', 'two_spheres', 'noise')
SAMPLED = ['image_' + n for n in PICTURES] + ['grid_' + n for n in GRIDS]

# Cases made for a state that no other case reaches.
#   march_at_min_step: a support ray that is UNRESOLVED after MAX_STEPS = 48 passes.  supports_ref.py: a ray advances by
#   max(v, min_step) per pass, so 48 passes cover at least 48 * START = 1.6 and a ray is left marching only where the field stays
#   below min_step over that length without turning negative -- no solid model does that along an oblique ray.  This one does on
#   purpose: plates 0.01 thick, 0.07 apart, that contain the support direction.  Between two plates the field is at most 0.03 <
#   START, and a downward ray stays between them: it creeps by min_step until the bed (a BED ray with dozens of steps) or until
#   the steps run out (UNRESOLVED).
EXTRA = {
    'march_at_min_step': "f = slab(x0=-0.005, x1=0.005).repeat((0.07, 0, 0)).rotate(np.arctan2(0.3, 0.5), Z)",
}

CASES = list(fixtures.FIXTURES) + list(fixtures.SLOT_FIXTURES) + [n for n in param_cases.CASES if n not in RAISES] + SAMPLED + list(EXTRA)
assert len(set(CASES)) == len(CASES) and not set(fixtures.FIXTURES) & set(param_cases.CASES)

PROBES = ('normals', 'thickness', 'supports', 'deviation', 'snap', 'render')

# ---- the fixed parameters of the probes ------------------------------------------------------------------------------------
N_AXIS = 24
AX = np.arange(N_AXIS) * (3.2 / N_AXIS) - 1.6         # the checker's meshing grid, per axis
MAX_TRIS, N_RANDOM = 300, 33
NORMAL_EPS = 1e-4
START = 3.2 / N_AXIS / 4                               # = min_step: a quarter of the grid step
T_FAR = 4.0
MAX_STEPS = 48                                         # (keeps a definition to about 70 evaluator calls)
THICKNESS = dict(normal_eps=NORMAL_EPS, start=START, min_step=START, t_far=T_FAR, max_steps=MAX_STEPS, refine=16)
ORDER = 2
SNAP = dict(eps=1e-4, tol=1e-5, max_move=0.1, iters=4)
DIRECTION = overhang_ref.normalise([(0.3, -0.5, 0.8)])[0]
SUPPORTS = dict(sin_limit=overhang_ref.sin_limit_of(45), bed_tol=0.0, start=START, min_step=START, max_steps=MAX_STEPS, refine=16)
WIDTH, HEIGHT = 45, 19                                 # ragged 8 x 8 tiles in both directions
RENDER_BOUNDS = ((-1.6,) * 3, (1.6,) * 3)              # fixed: estimate_bounds fails for a model that is NaN everywhere


def _pictures():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_texture', os.path.join(ROOT, 'tools', 'make_golden_texture.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.pictures()


def _grids():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_custom', os.path.join(ROOT, 'tools', 'make_golden_custom.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.grids()


def build(name, ns):
    """the model of case `name` over the ``from sdf import *`` namespace `ns`"""
    if name in fixtures.FIXTURES or name in fixtures.SLOT_FIXTURES:
        return fixtures.build(name, ns)
    if name in param_cases.CASES:
        return param_cases.build(name, ns)
    if name in EXTRA:
        scope = dict(ns)
        exec(EXTRA[name], scope)
        return scope['f']
    kind, _, which = name.partition('_')
    if kind == 'image' and which in PICTURES:
        arr, kw = _pictures()[which]
        return ns['image'](arr, **kw).extrude(0.4)
    if kind == 'grid' and which in GRIDS:
        from sdf_amd import mesh
        X, Y, Z, A, background, box = _grids()[which]
        return mesh.grid_sdf((X, Y, Z), A, background, box)
    raise KeyError(name)


_models = {}


def model(name, ns):
    """(model, tape), built and lowered once per case"""
    if name not in _models:
        from sdf_amd import tape
        f = build(name, ns)
        _models[name] = (f, tape.lower(f))
    return _models[name]


def swept(name, ns):
    """a case goes through the kernels unless its tape reads user closures"""
    return not model(name, ns)[1].externs


def axes(name, ns):
    """the meshing grid of a case: AX on every axis; for a sampled-leaf model, whose surface is small, N_AXIS samples over its own
    estimated bounds (the checker's)"""
    if name not in SAMPLED:
        return AX, AX, AX
    import oracle
    lo, hi = oracle.estimate_bounds(model(name, ns)[0])
    return tuple(np.arange(N_AXIS) * ((b - a) / N_AXIS) + a for a, b in zip(lo, hi))


_inputs = {}


def inputs(name, ns):
    """(soup (T, 9) float64, welded points (U, 3) float64), read-only, made once per case"""
    if name not in _inputs:
        import oracle
        X, Y, Z = axes(name, ns)
        g = oracle.generate(model(name, ns)[0], X, Y, Z, 32, True).points.reshape(-1, 9)
        g = g[np.isfinite(g).all(axis=1)]
        k = max(1, math.ceil(len(g) / MAX_TRIS))
        g = g[::k][:MAX_TRIS]
        soup = np.concatenate([g, np.random.RandomState(93).uniform(-1.5, 1.5, (N_RANDOM, 9))]) + 0.0      # (+ 0.0: no -0.0, which np.unique
        pts = np.unique(soup.reshape(-1, 3), axis=0)                                                        # and a sort by bits order apart)
        soup.setflags(write=False)
        pts.setflags(write=False)
        _inputs[name] = (soup, pts)
    return _inputs[name]


def render_setup():
    """(frame, the keyword parameters of `render_ref.render` and `Engine.render_buffers`)"""
    import importlib
    R = importlib.import_module('sdf_amd.render')          # (the package attribute `sdf_amd.render` is the function)
    frame, t_near, t_far, radius = R.camera(RENDER_BOUNDS, WIDTH, HEIGHT)
    return frame, dict(t_near=t_near, t_far=t_far, hit_eps=1e-4 * radius, step_scale=1.0, normal_eps=1e-4 * radius, max_steps=MAX_STEPS, refine=8)


# ---- the definitions, every output as a named array ------------------------------------------------------------------------
def define(probe, ev, soup, pts):
    """the outputs of one probe by its definition over the evaluator `ev(P) -> (N,) float64`: a dict name -> array, in the
    order and under the names that `test_probe_sweep_gpu.device` gives the kernel's"""
    if probe == 'normals':
        n, n_flat = normals_ref.vertex_normals(ev, pts, NORMAL_EPS)
        return {'normal': n, 'n_flat': np.int64(n_flat)}
    if probe == 'thickness':
        th, status, steps = thickness_ref.thickness(ev, pts, **THICKNESS)
        return {'thickness': th, 'status': status, 'steps': steps}
    if probe == 'supports':
        r = supports_ref.supports(ev, soup.reshape(-1, 3, 3), DIRECTION, **SUPPORTS)
        out = {k: r[k] for k in ('triangle', 'height', 'status', 'steps', 'origin', 'sums', 'counts')}
        out['lo'], out['hi'] = np.float64(r['lo']), np.float64(r['hi'])
        return out
    if probe == 'deviation':
        dev, at, sumsq = deviation_ref.deviation(ev, soup.reshape(-1, 3, 3), ORDER)
        return {'dev': dev, 'at': at, 'sumsq': sumsq}
    if probe == 'snap':
        q, status, residual, evals = deviation_ref.snap(ev, pts, **SNAP)
        return {'points': q, 'status': status, 'residual': residual, 'evals': evals}
    if probe == 'render':
        frame, par = render_setup()
        r = render_ref.render(ev, frame, WIDTH, HEIGHT, **par)
        return {k: r[k] for k in ('depth', 'normal', 'steps', 'status')}
    raise KeyError(probe)


# ---- what a tape holds ----------------------------------------------------------------------------------------------------
# the constant (past K) that holds the easing id of the ops that call ease_apply (csrc/sdf_interp.h)
EASE_CONST = {'BEND_LINEAR': 10, 'WRAP_AROUND': 10, 'BEND_RADIAL': 3, 'TRANS_LIN_PRE': 7, 'TRANS_RAD_PRE': 2, 'EXTTO_PRE': 1}
# the ops whose value is folded into the accumulator through `post`: the leaves and COMB
def _folds(op):
    return op.startswith('L_') or op == 'COMB'


def census(t):
    """(opcodes, post codes, easing ids) that tape t holds: the op byte of every instruction's first word; the RL / SV / PD
    prefixes counted as LOAD_P / SAVE_P / PUSH_D, whose work they do; `post` of the instructions that fold a value; the easing
    id of the instructions that take one"""
    from sdf_amd import tape
    ops, posts, eases = set(), set(), set()
    for i in range(t.n_instr):
        w0, w1 = int(t.code[2 * i]), int(t.code[2 * i + 1])
        op = tape.OP_NAMES[w0 & 255]
        ops.add(op)
        if w0 & tape.RL_FLAG:
            ops.add('LOAD_P')
        if w0 & tape.SV_FLAG:
            ops.add('SAVE_P')
        if w0 & tape.PD_FLAG:
            ops.add('PUSH_D')
        if _folds(op):
            posts.add((w0 >> 8) & 7)
        if op in EASE_CONST:
            eases.add(int(t.consts[(w1 & tape.COFF_MASK) + 1 + EASE_CONST[op]]))
    return ops, posts, eases
