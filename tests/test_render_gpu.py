"""The device sphere tracer (csrc/sdf_render.hip, `Engine.render_buffers`, `f.render`): every buffer bit-identical to the NumPy
restatement (tests/render_ref.py) run over the same interpreter (`Engine.eval_points`) and, for the models without libm calls,
over the CPU checker; the entry points and the refusals.  Every refusal is decided on the host before a launch; no test
repeats a device call that failed."""
import ctypes
import importlib

import numpy as np
import pytest

import fixtures
import render_ref as ref
from sdf_amd import engine

pytestmark = pytest.mark.gpu

R = importlib.import_module('sdf_amd.render')       # (the package attribute `sdf_amd.render` is the function)
# plain family, trig family (twice), smooth unions, the longest tape of the examples, the largest register files
# (opcode coverage lives in the sweep, tests/test_probe_sweep_gpu.py: every tape of the suite goes through this kernel there; these few
# models walk the kernel's own states)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'ex_knurling', 'slots_plain_8_8_p8d8')
# whole tiles; ragged in both directions; one tile; one pixel; one row of tiles; one column of tiles
SIZES = ((48, 32), (45, 19), (8, 8), (1, 1), (64, 1), (1, 64))
LIBM_FREE = ('ex_example', 'ex_blobby', 'torus')
_models = {}


def model(name, ns, eng):
    """(model, bounds) -- the bounds estimated once per model"""
    if name not in _models:
        f = fixtures.build(name, ns)
        _models[name] = (f, eng.estimate_bounds(f))
    return _models[name]


def setup(bounds, w, h, ortho=False, **over):
    frame, t_near, t_far, radius = R.camera(bounds, w, h, ortho=ortho)
    p = dict(t_near=t_near, t_far=t_far, hit_eps=1e-4 * radius, step_scale=1.0, normal_eps=1e-4 * radius, max_steps=256, refine=8)
    p.update(over)
    return frame, p


def same_bits(got, want):
    for key, dtype in (('depth', np.float64), ('normal', np.float64), ('steps', np.int32), ('status', np.uint8)):
        g, w = got[key], want[key]
        assert g.dtype == dtype and w.dtype == dtype and g.shape == w.shape, (key, g.dtype, g.shape, w.shape)
        bad = ref.bits(g) != ref.bits(w)
        assert not bad.any(), '%s: %d of %d values differ, first at %s: %r != %r' % (
            key, bad.sum(), bad.size, np.argwhere(bad)[0], g[bad][0], w[bad][0])


def check(eng, f, bounds, w, h, ev=None, ortho=False, **over):
    frame, p = setup(bounds, w, h, ortho, **over)
    got = eng.render_buffers(f, frame, w, h, **p)
    want = ref.render(ev or (lambda P: eng.eval_points(f, P)), frame, w, h, **p)
    same_bits(got, want)
    return got


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', MODELS)
def test_buffers_are_bit_identical_to_the_restatement(name, size, ns, eng):
    f, bounds = model(name, ns, eng)
    got = check(eng, f, bounds, *size)
    if size == (48, 32):
        hit = got['status'] == 1
        assert hit.any() and not hit.all() and got['steps'].max() < 256


@pytest.mark.parametrize('size', ((48, 32), (45, 19)), ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', LIBM_FREE)
def test_buffers_are_bit_identical_to_the_restatement_over_the_checker(name, size, ns, eng, oracle_lib):
    f, bounds = model(name, ns, eng)
    check(eng, f, bounds, *size, ev=lambda P: oracle_lib.evaluate(f, P))


@pytest.mark.parametrize('setting', ('ortho', 'step_scale', 'no_refine', 'five_steps'))
@pytest.mark.parametrize('name', ('ex_example', 'twist'))
def test_other_settings(name, setting, ns, eng):
    f, bounds = model(name, ns, eng)
    over = {'ortho': dict(ortho=True), 'step_scale': dict(step_scale=0.5), 'no_refine': dict(refine=0), 'five_steps': dict(max_steps=5)}[setting]
    got = check(eng, f, bounds, 45, 19, **over)
    if setting == 'five_steps':
        out = (got['steps'] == 5) & (got['status'] == 0)                     # rays that ran out: misses with every step spent
        assert out.any() and np.isinf(got['depth'][out]).all() and got['steps'].max() == 5
    else:
        assert (got['status'] == 1).any()


def test_render_writes_a_png(ns, eng, tmp_path):
    from PIL import Image
    f, _ = model('ex_example', ns, eng)
    path = str(tmp_path / 'preview.png')
    img = f.render(path, width=64, height=48)
    assert img.dtype == np.uint8 and img.shape == (48, 64, 3)
    with Image.open(path) as im:
        assert im.size == (64, 48) and im.mode == 'RGB'
        back = np.array(im)
    assert np.array_equal(back, img) and len(np.unique(back.reshape(-1, 3), axis=0)) >= 2
    buf = R.render_buffers(f, 64, 48)
    assert np.array_equal(R.shade(buf, buf['frame']), img)
    assert np.array_equal(ns['render'](f, width=64, height=48), img)


def _lib_call(eng, handle, frame, w, h, params, max_steps=64, refine=8, null=None):
    out = {'depth': np.full((8, 8), 7.0), 'normal': np.full((8, 8, 3), 7.0), 'steps': np.full((8, 8), 7, np.int32), 'status': np.full((8, 8), 7, np.uint8)}
    f64, i32, u8 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    ptr = {'frame': None if frame is None else frame.ctypes.data_as(f64), 'params': None if params is None else params.ctypes.data_as(f64),
           'depth': out['depth'].ctypes.data_as(f64), 'normal': out['normal'].ctypes.data_as(f64), 'steps': out['steps'].ctypes.data_as(i32),
           'status': out['status'].ctypes.data_as(u8)}
    if null:
        ptr[null] = None
    rc = eng.lib.sdf_render_host(handle, ptr['frame'], w, h, ptr['params'], max_steps, refine, ptr['depth'], ptr['normal'], ptr['steps'], ptr['status'])
    assert all((a == 7).all() for a in out.values())                         # a refused call writes nothing
    return rc


def test_refusals_and_the_context_stays_intact(ns, eng):
    f, bounds = model('ex_example', ns, eng)
    frame, p = setup(bounds, 8, 8)
    check(eng, f, bounds, 8, 8)
    closure = fixtures.build('custom_leaf_in_example', ns)
    closure_tape = eng.tape_for(closure)                                     # (uploaded before the free memory is read)

    def free():
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert eng.lib.sdf_device_mem_info(0, ctypes.byref(a), ctypes.byref(b)) == 0
        return a.value
    f0 = free()
    nan_frame, inf_frame = frame.copy(), frame.copy()
    nan_frame[4], inf_frame[17] = np.nan, np.inf
    bad = [dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 13, height=(1 << 13) + 1), dict(width=1 << 40, height=1 << 40),
           dict(max_steps=0), dict(refine=-1), dict(frame=nan_frame), dict(frame=inf_frame), dict(frame=frame[:17]),
           dict(t_near=np.nan), dict(t_far=np.inf), dict(hit_eps=0.0), dict(hit_eps=-1e-3), dict(hit_eps=np.nan), dict(normal_eps=0.0),
           dict(normal_eps=-1.0), dict(step_scale=0.0), dict(step_scale=1.0 + 1e-12), dict(step_scale=-0.5), dict(step_scale=np.inf),
           dict(t_near=2.0, t_far=1.0)]
    for kw in bad:
        args = dict(p, frame=frame, width=8, height=8)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.render_buffers(f, **args)
    with pytest.raises(ValueError, match='closure'):
        eng.render_buffers(closure, frame, 8, 8, **p)
    with pytest.raises(ValueError, match='closure'):
        closure.render(width=8, height=8, bounds=bounds)
    old = eng.precision
    try:
        eng.precision = engine.PRECISION_F32
        with pytest.raises(ValueError, match='float32'):
            eng.render_buffers(f, frame, 8, 8, **p)
    finally:
        eng.precision = old
    # the C entry point checks on its own, and says why
    tape = eng.tape_for(f)                                                   # (held: the handle lives as long as this object)
    h = tape.handle
    par = np.array([p['t_near'], p['t_far'], p['hit_eps'], 1.0, p['normal_eps']])

    def with_par(i, v):
        q = par.copy()
        q[i] = v
        return q
    for null in ('frame', 'params', 'depth', 'normal', 'steps', 'status'):
        assert _lib_call(eng, h, frame, 8, 8, par, null=null) == 2 and b'NULL' in eng.lib.sdf_last_error()
    assert _lib_call(eng, None, frame, 8, 8, par) == 2
    assert _lib_call(eng, h, frame, 0, 8, par) == 2 and _lib_call(eng, h, frame, 8, -1, par) == 2
    assert _lib_call(eng, h, frame, 1 << 13, (1 << 13) + 1, par) == 2 and b'2^26' in eng.lib.sdf_last_error()
    assert _lib_call(eng, h, frame, 8, 8, par, max_steps=0) == 2 and _lib_call(eng, h, frame, 8, 8, par, refine=-1) == 2
    assert _lib_call(eng, h, nan_frame, 8, 8, par) == 2 and _lib_call(eng, h, inf_frame, 8, 8, par) == 2
    for i, v in ((0, np.nan), (1, np.inf), (2, 0.0), (2, -1.0), (4, 0.0), (3, 0.0), (3, 1.5), (3, np.nan)):
        assert _lib_call(eng, h, frame, 8, 8, with_par(i, v)) == 2, (i, v)
    assert _lib_call(eng, h, frame, 8, 8, with_par(1, p['t_near'] - 1.0)) == 2 and b't_far' in eng.lib.sdf_last_error()
    assert _lib_call(eng, closure_tape.handle, frame, 8, 8, par) == 2 and b'closures' in eng.lib.sdf_last_error()
    assert free() == f0
    # the context is intact, and a call holds nothing once it has returned
    check(eng, f, bounds, 8, 8)
    check(eng, f, bounds, 45, 19)
    assert free() == f0
