"""The device distance texture (csrc/sdf_edt.hip, `text(..., edt='device')` / `image(..., edt='device')`): bit-exact against
the NumPy restatement (tests/edt_ref.py) on every pixel of every case, end to end through the texture leaf, and its refusals.
Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
import ctypes
import hashlib
import importlib

import numpy as np
import pytest

import edt_ref as ref
from sdf_amd import tape

pytestmark = pytest.mark.gpu

T = importlib.import_module('sdf_amd.text')        # (the package attribute `sdf_amd.text` is the function)
CASES = ref.cases()
GOLDEN = ref.golden()


def same_bits(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = ref.bits(got) != ref.bits(want)
    assert not bad.any(), '%d of %d pixels differ, first at %s: %r != %r' % (
        bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


@pytest.mark.parametrize('name', sorted(CASES))
def test_texture_is_bit_identical_to_the_restatement(name, eng):
    m = CASES[name]
    want = ref.distance_texture(m)
    same_bits(eng.distance_texture(m), want)
    same_bits(eng.distance_texture(m.astype(np.uint8) * 255), want)          # any non-zero byte is True
    same_bits(T.distance_texture(m, 'device'), want)
    same_bits(eng.distance_texture(np.asfortranarray(m)), want)              # not C-contiguous


@pytest.mark.parametrize('name', sorted(GOLDEN))
def test_texture_is_bit_identical_to_the_recorded_scipy_textures(name, eng):
    m, tex = GOLDEN[name]
    same_bits(eng.distance_texture(m), tex)


def stress_masks():
    """masks that stress the kernels' shape; (mask, which restatement reaches it)"""
    rng = np.random.RandomState(777)
    out = {}
    out['line_1x5000'] = (rng.uniform(size=(1, 5000)) < 0.01, 'brute')
    out['line_5000x1'] = (rng.uniform(size=(5000, 1)) < 0.99, 'brute')
    longest = np.zeros((1, 46340), bool)                    # the longest line there is, and squared distances up to 46339^2 < 2^31
    longest[0, 0] = True
    out['line_1x46340'] = (longest, 'brute')
    corner = np.ones((700, 4700), bool)
    corner[699, 0] = False                                  # the largest distances and the longest searches
    out['corner_700x4700'] = (corner, 'brute')
    tall = np.zeros((1100, 300), bool)
    tall[0, 299] = True
    out['corner_tall_1100x300'] = (tall, 'brute')
    out['dense_2048x2048'] = (rng.uniform(size=(2048, 2048)) < 0.5, 'separable')
    out['r_67x1031'] = (rng.uniform(size=(67, 1031)) < 0.3, 'separable')         # off every multiple of 64 and of the 16-line tile
    out['r_1031x67'] = (rng.uniform(size=(1031, 67)) < 0.7, 'separable')
    out['sparse_150x3001'] = (rng.uniform(size=(150, 3001)) < 0.0005, 'separable')   # whole 64-pixel words without a True pixel
    out['r_1300x1500'] = (rng.uniform(size=(1300, 1500)) < 0.002, 'separable')   # 8 lines per workgroup
    blob = np.zeros((513, 2111), bool)
    yy, xx = np.mgrid[0:513, 0:2111]
    for _ in range(12):
        cy, cx, r = rng.uniform(0, 513), rng.uniform(0, 2111), rng.uniform(20, 160)
        blob[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] ^= True
    out['blobs_513x2111'] = (blob, 'separable')
    for m, _ in out.values():
        m.flat[0] |= not m.any()                            # both classes, whatever the draw
    return out


STRESS = stress_masks()


@pytest.mark.parametrize('name', sorted(STRESS))
def test_kernel_shapes(name, eng):
    m, how = STRESS[name]
    assert m.any() and not m.all()
    want = ref.distance_texture(m) if how == 'brute' else ref.distance_texture_separable(m)
    same_bits(eng.distance_texture(m), want)


def test_device_texture_equals_scipy_where_it_is_installed(eng):
    pytest.importorskip('scipy')
    for name in ('corner_700x4700', 'r_67x1031', 'blobs_513x2111', 'line_5000x1'):
        m = STRESS[name][0]
        same_bits(eng.distance_texture(m), T.distance_texture(m, 'host'))


def _soup_sha(f):
    pts = f.generate(samples=2 ** 15, verbose=False)
    assert len(pts) > 300 and np.isfinite(pts).all()
    return hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest()


def _same_constants(f, g):
    a, b = tape.lower(f), tape.lower(g)
    assert np.array_equal(a.code, b.code)
    assert np.array_equal(np.asarray(a.consts).view(np.int64), np.asarray(b.consts).view(np.int64))


def test_image_end_to_end(ns, eng):
    rng = np.random.RandomState(31337)
    yy, xx = np.mgrid[0:96, 0:80]
    pic = np.zeros((96, 80), np.uint8)
    for _ in range(9):
        cx, cy, r = rng.uniform(10, 70), rng.uniform(10, 86), rng.uniform(4, 14)
        pic[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = 255
    f = ns['image'](pic, height=2.0, edt='device')
    mask = T._mask(T.PIXELS, 0, 0, T._as_pil(pic).convert('L'))[0]
    want = T.texture_sdf(ref.distance_texture(mask), height=2.0)
    _same_constants(f, want)
    assert _soup_sha(f.extrude(0.4)) == _soup_sha(want.extrude(0.4))
    try:
        import scipy  # noqa: F401
    except ImportError:
        return
    _same_constants(f, ns['image'](pic, height=2.0))
    _same_constants(f, ns['image'](pic, height=2.0, edt='host'))


def test_text_end_to_end(ns, eng):
    font = ref.dejavu()
    if font is None:
        pytest.skip('matplotlib (its bundled DejaVuSans.ttf) is not installed')
    f = ns['text'](font, 'Hi', width=3.0, points=96, edt='device')
    canvas, pad = T._canvas(font, 'Hi', 96)
    mask, px, py = T._mask(T.PIXELS, pad[0], pad[1], canvas)
    want = T.texture_sdf(ref.distance_texture_separable(mask), width=3.0, px=px, py=py)
    _same_constants(f, want)
    assert _soup_sha(f.extrude(0.5)) == _soup_sha(want.extrude(0.5))
    try:
        import scipy  # noqa: F401
    except ImportError:
        return
    _same_constants(f, ns['text'](font, 'Hi', width=3.0, points=96))
    old = T.EDT
    try:
        T.EDT = 'device'                                    # the module default, for calls that do not say
        _same_constants(f, ns['text'](font, 'Hi', width=3.0, points=96))
    finally:
        T.EDT = old


def _lib_call(eng, mask, rows, cols, out):
    return eng.lib.sdf_distance_texture_host(eng.ctx, None if mask is None else mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), rows, cols,
                                             None if out is None else out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))


def test_refusals_raise_and_nothing_is_held(eng):
    m = CASES['frame']
    eng.distance_texture(m)

    def free():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert eng.lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    f0 = free()
    big = np.zeros((46341, 1), bool)                        # 46341^2 + 1 >= 2^31
    big[7] = True
    for bad in (np.ones((3, 4), bool), np.zeros((3, 4), bool), np.ones((1, 1), bool), np.zeros((0, 4), bool), np.zeros((4, 0), bool),
                np.zeros(7, bool), np.zeros((2, 3, 4), bool), big, big.T):
        with pytest.raises(ValueError):
            eng.distance_texture(bad)
        with pytest.raises(ValueError):
            T.distance_texture(bad, 'device')
    with pytest.raises(ValueError):
        importlib.import_module('sdf_amd').image(np.full((20, 30), 255, np.uint8), edt='device')      # an all-white picture: one class
    # the C entry point checks on its own, too, and says why
    u8 = m.astype(np.uint8)
    out = np.full(m.shape, 7.0)
    assert _lib_call(eng, None, 40, 60, out) == 2 and _lib_call(eng, u8, 40, 60, None) == 2
    assert _lib_call(eng, u8, 0, 60, out) == 2 and b'empty mask' in eng.lib.sdf_last_error()
    assert _lib_call(eng, u8, 40, -1, out) == 2
    assert _lib_call(eng, u8, 46341, 1, out) == 2 and b'2^31' in eng.lib.sdf_last_error()
    assert _lib_call(eng, u8, 1 << 40, 1 << 40, out) == 2
    assert _lib_call(eng, u8, 16385, 16385, out) == 2 and b'shorter side' in eng.lib.sdf_last_error()     # (the mask is not read)
    assert _lib_call(eng, np.ones((40, 60), np.uint8), 40, 60, out) == 2 and b'True' in eng.lib.sdf_last_error()
    assert np.all(out == 7.0)                               # a refused call writes nothing
    assert free() == f0
    # device memory: equal before and after 50 calls of different sizes
    rng = np.random.RandomState(5)
    for i in range(50):
        a = rng.uniform(size=(20 + 7 * i, 300 - 5 * i)) < 0.3
        a[0, 0], a[-1, -1] = True, False
        eng.distance_texture(a)
    assert free() == f0
