"""The definition of the sphere-traced render buffers (tests/render_ref.py) over the CPU checker, and the host side of
`render`: the ABI entry, the camera, the shading and the entry points.  No GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import fixtures
import render_ref as ref
from sdf_amd import engine

R = importlib.import_module('sdf_amd.render')       # (the package attribute `sdf_amd.render` is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 32
MAX_STEPS, REFINE = 256, 8
MODELS = ('sphere', 'torus', 'ex_example', 'ex_blobby', 'twist', 'ex_knurling')
EXACT = ('sphere', 'torus', 'ex_example')           # true distance fields: a step never passes the surface
_traced = {}


def traced(name, ns, oracle):
    """(model, frame, params, buffers) of the default view at 48 x 32, traced once per model over the CPU checker"""
    if name not in _traced:
        f = fixtures.build(name, ns)
        frame, t_near, t_far, radius = R.camera(oracle.estimate_bounds(f), W, H)
        p = dict(t_near=t_near, t_far=t_far, hit_eps=1e-4 * radius, step_scale=1.0, normal_eps=1e-4 * radius, max_steps=MAX_STEPS, refine=REFINE)
        buf = ref.render(lambda P: oracle.evaluate(f, P), frame, W, H, **p)
        for a in buf.values():
            a.setflags(write=False)
        _traced[name] = (f, frame, p, buf)
    return _traced[name]


def test_abi_has_the_entry_point():
    assert 'sdf_render_host' in engine.ABI and engine.ABI_VERSION >= 13
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_render_host\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == engine.ABI_VERSION
    assert callable(getattr(engine.Engine, 'render_buffers'))


def test_entry_point_refuses_a_null_tape_without_a_device():
    lib = engine.load_library()
    d = np.zeros(18)
    p64 = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    s = np.zeros(4, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    u = np.zeros(4, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.sdf_render_host(None, p64, 1, 1, p64, 8, 0, p64, p64, s, u) == 2
    assert b'sdf_render_host' in lib.sdf_last_error()


@pytest.mark.parametrize('name', MODELS)
def test_properties_of_the_restatement(name, ns, oracle_lib):
    f, frame, p, buf = traced(name, ns, oracle_lib)
    depth, normal, steps, status = (buf[k] for k in ('depth', 'normal', 'steps', 'status'))
    assert depth.shape == (H, W) and normal.shape == (H, W, 3) and steps.dtype == np.int32 and status.dtype == np.uint8
    hit = status == 1
    assert hit.any() and not hit.all()
    assert steps.min() >= 1 and steps.max() < MAX_STEPS                      # no ray runs out
    P, idx = ref.hit_points(buf, frame)
    v = oracle_lib.evaluate(f, P).reshape(-1)
    assert (v < p['hit_eps']).all(), v.max()
    if name in EXACT:
        assert (v >= 0).all(), v.min()
    ln = np.sqrt((normal[hit] ** 2).sum(axis=1))
    assert (np.abs(ln - 1) <= 4 * np.spacing(1.0)).all(), np.abs(ln - 1).max()
    assert np.isinf(depth[~hit]).all() and (depth[~hit] > 0).all() and not normal[~hit].any()
    assert (depth[hit] >= p['t_near']).all() and (depth[hit] <= p['t_far']).all()


def test_sphere_hits_where_the_ray_meets_it(ns, oracle_lib):
    f, frame, p, buf = traced('sphere', ns, oracle_lib)
    O, D = ref.rays(frame, W, H)
    # the distance at which the ray passes the centre (the origin): |O - (O . D) D|
    along = (O * D).sum(axis=1)
    closest = np.sqrt(((O - along[:, None] * D) ** 2).sum(axis=1))
    status = buf['status'].reshape(-1)
    eps = p['hit_eps']
    assert (status[closest < 1 - eps] == 1).all() and (status[closest > 1 + eps] == 0).all()
    assert (closest < 1 - eps).sum() > 100 and (closest > 1 + eps).sum() > 100
    P, idx = ref.hit_points(buf, frame)
    r = np.sqrt((P ** 2).sum(axis=1))
    assert (np.abs(r - 1) <= eps).all(), np.abs(r - 1).max()
    # central differences of an exact sphere field are exact to O(h^2) = 1e-8 here; 1e-6 is two decades of margin
    n = buf['normal'].reshape(-1, 3)[idx]
    assert np.abs(n - P / r[:, None]).max() <= 1e-6


def test_a_ray_that_starts_inside(ns, oracle_lib):
    f = fixtures.build('sphere', ns)
    frame, t_near, t_far, radius = R.camera(((-1, -1, -1), (1, 1, 1)), 5, 3, eye=(0, 0, 0), target=(1, 0, 0))
    assert t_near == 0.0
    calls = []

    def ev(P):
        calls.append(len(P))
        return oracle_lib.evaluate(f, P)
    buf = ref.render(ev, frame, 5, 3, t_near, t_far, 1e-4, 1.0, 1e-4, max_steps=64, refine=8)
    assert (buf['status'] == 1).all() and (buf['depth'] == t_near).all() and (buf['steps'] == 1).all()
    assert calls == [15] + [15] * 6                                          # one march step, no refinement, the normal


def test_camera_centre_ray_passes_through_the_target():
    bounds = ((-1.0, -2.0, -0.5), (3.0, 1.0, 2.5))
    for kw in ({}, {'target': (0.3, -0.2, 0.1)}, {'eye': (4.0, 5.0, 6.0)}, {'ortho': True}, {'fov': 60.0, 'up': (0, 1, 0)}):
        frame, t_near, t_far, radius = R.camera(bounds, 31, 17, **kw)
        O, D = ref.rays(frame, 31, 17)
        c = 8 * 31 + 15
        target = np.asarray(kw.get('target', (1.0, -0.5, 1.0)), float)
        to = target - O[c]
        off = to - np.dot(to, D[c]) * D[c]
        assert np.sqrt(np.dot(off, off)) <= 1e-12 * (1 + np.sqrt(np.dot(to, to))), kw
        assert np.dot(to, D[c]) > 0
        assert np.allclose(np.sqrt((D ** 2).sum(axis=1)), 1.0, rtol=0, atol=1e-15)
        assert radius == pytest.approx(np.sqrt(16 + 9 + 9) / 2) and 0 <= t_near < t_far


def test_camera_orthographic_rays_are_parallel():
    frame, *_ = R.camera(((-1, -1, -1), (1, 1, 1)), 20, 10, ortho=True)
    O, D = ref.rays(frame, 20, 10)
    assert (ref.bits(D) == ref.bits(D[0])).all()
    assert not frame[12:].any() and frame[3:9].any()
    assert len(np.unique(O, axis=0)) == 200
    pframe, *_ = R.camera(((-1, -1, -1), (1, 1, 1)), 20, 10)
    assert not pframe[3:9].any() and pframe[12:].any()


@pytest.mark.parametrize('ortho', (False, True))
@pytest.mark.parametrize('size', ((64, 48), (48, 64), (33, 33)))
def test_camera_default_view_frames_the_bounds(size, ortho):
    w, h = size
    lo, hi = np.array((-1.0, -2.0, -0.5)), np.array((3.0, 1.0, 2.5))
    frame, t_near, t_far, radius = R.camera((lo, hi), w, h, ortho=ortho)
    o0, ou, ov, c, du, dv = frame.reshape(6, 3)
    for corner in np.array(np.meshgrid(*zip(lo, hi))).reshape(3, -1).T:
        # the pixel coordinates (i, j) whose ray passes through the corner: a 3 x 3 system per corner
        if ortho:
            i, j, t = np.linalg.solve(np.stack([ou, ov, c], axis=1), corner - o0)
        else:
            a, b, s = np.linalg.solve(np.stack([du, dv, -(corner - o0)], axis=1), -c)     # c + i du + j dv = s (corner - o0)
            i, j, t = a, b, 1 / s
        assert -0.5 <= i <= w - 0.5 and -0.5 <= j <= h - 0.5, (corner, i, j)
        assert t > 0


def test_camera_refuses_what_has_no_view():
    b = ((-1, -1, -1), (1, 1, 1))
    for kw in ({'eye': (0, 0, 0), 'target': (0, 0, 0)}, {'fov': 0}, {'fov': 180}):
        with pytest.raises(ValueError):
            R.camera(b, 8, 8, **kw)
    with pytest.raises(ValueError):
        R.camera(b, 0, 8)
    with pytest.raises(ValueError):
        R.camera(((0, 0, 0), (0, 0, 0)), 8, 8)
    R.camera(b, 8, 8, eye=(0, 0, 5), target=(0, 0, 0))                       # looking along `up` still has a horizon


def test_shade_a_hand_made_buffer():
    frame = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 0, 0])        # every ray looks down -z: the headlight is +z
    normal = np.zeros((2, 2, 3))
    normal[0, 0] = (0, 0, 1)                             # faces the light
    normal[0, 1] = (0, 0.6, 0.8)
    normal[1, 0] = (0, 0, -1)                            # faces away: ambient only
    buf = {'status': np.array([[1, 1], [1, 0]], np.uint8), 'normal': normal, 'depth': np.ones((2, 2)), 'steps': np.ones((2, 2), np.int32)}
    img = R.shade(buf, frame, color=(1.0, 0.5, 0.2), background=(0.0, 1.0, 0.4), ambient=0.25)
    assert img.dtype == np.uint8 and img.shape == (2, 2, 3)
    assert img[0, 0].tolist() == [255, 128, 51]                              # 255 * (1, 0.5, 0.2) * 1.0, rounded to even
    assert img[0, 1].tolist() == [217, 108, 43]                              # * (0.25 + 0.75 * 0.8) = 0.85
    assert img[1, 0].tolist() == [64, 32, 13]                                # * 0.25
    assert img[1, 1].tolist() == [0, 255, 102]                               # a miss takes the background
    side = R.shade(buf, frame, light=(0, 5, 0), color=(1.0, 0.5, 0.2), background=(0.0, 1.0, 0.4), ambient=0.25)
    assert side[0, 0].tolist() == [64, 32, 13] and side[0, 1].tolist() == [178, 89, 36] and side[1, 1].tolist() == [0, 255, 102]


def test_render_refuses_a_2d_model(ns):
    with pytest.raises(TypeError, match='extrude'):
        R.render(ns['circle'](1))
    with pytest.raises(TypeError, match='extrude'):
        R.render_buffers(ns['hexagon'](1), 8, 8)
    assert ns['render'] is R.render and callable(ns['sphere'](1).render)


def test_lockstep_share():
    steps = np.ones((16, 16), np.int32)
    assert ref.lockstep_share(steps) == 1.0
    steps[0, 0] = 4                                       # one tile of four now waits for one ray: 64 * (4 + 1 + 1 + 1) slots
    assert ref.lockstep_share(steps) == pytest.approx((256 + 3) / (64 * 7))
    assert ref.lockstep_share(np.ones((1, 64), np.int32), tile=(1, 64)) == 1.0
