"""The NumPy restatement of the device distance texture (tests/edt_ref.py) against scipy and against its goldens, and the
host side of `edt=`: the option, its default, the ABI entry and that 'device' mode never imports scipy.  No GPU."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import edt_ref as ref
from sdf_amd import engine

T = importlib.import_module('sdf_amd.text')        # (the package attribute `sdf_amd.text` is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_equals_scipy(name):
    pytest.importorskip('scipy')
    m = CASES[name]
    assert np.array_equal(ref.bits(ref.distance_texture(m)), ref.bits(T.distance_texture(m)))
    assert np.array_equal(ref.bits(ref.distance_texture(m)), ref.bits(T.distance_texture(m, 'host')))


def test_restatement_equals_scipy_on_rendered_text():
    pytest.importorskip('scipy')
    pytest.importorskip('PIL')
    font = ref.dejavu()
    if font is None:
        pytest.skip('matplotlib (its bundled DejaVuSans.ttf) is not installed')
    m = ref.rendered_mask(font, 'Hello', 64)
    assert m.any() and not m.all() and m.size > 4000
    want = ref.bits(T.distance_texture(m))
    assert np.array_equal(ref.bits(ref.distance_texture(m)), want)
    assert np.array_equal(ref.bits(ref.distance_texture_separable(m)), want)


@pytest.mark.parametrize('name', sorted(CASES))
def test_separable_form_equals_brute_force(name):
    m = CASES[name]
    D = ref.squared(m)
    assert D.dtype == np.int64 and D.min() >= 1
    assert np.array_equal(ref.squared_separable(m), D)
    assert np.array_equal(ref.squared_separable(m.T), D.T)


def test_brute_force_chunking_does_not_matter():
    m = CASES['r_37x53_50']
    assert np.array_equal(ref.squared(m, chunk=1000), ref.squared(m))


@pytest.mark.parametrize('name', sorted(ref.golden()))
def test_restatement_equals_the_recorded_scipy_textures(name):
    m, tex = ref.golden()[name]
    assert tex.dtype == np.float64 and tex.shape == m.shape
    assert np.array_equal(ref.bits(ref.distance_texture(m)), ref.bits(tex))
    assert np.array_equal(ref.bits(ref.distance_texture_separable(m)), ref.bits(tex))
    if name in CASES:
        assert np.array_equal(m, CASES[name])           # the generator still makes the recorded mask
    # the squared distances are integers, and the texture is the correctly rounded root of them
    D = np.rint(tex * tex).astype(np.int64)
    assert np.array_equal(np.sqrt(D.astype(np.float64)), np.abs(tex)) and np.array_equal(tex < 0, m)


def test_one_class_and_empty_masks_are_refused_by_the_restatement():
    for m in (np.ones((3, 4), bool), np.zeros((3, 4), bool), np.zeros((0, 4), bool), np.zeros(5, bool)):
        with pytest.raises(ValueError):
            ref.squared(m)
        with pytest.raises(ValueError):
            ref.squared_separable(m)


def test_edt_option_and_its_default():
    assert T.EDT == 'host'
    m = CASES['frame']
    for bad in ('bogus', '', None, 'Device', 1):
        with pytest.raises(ValueError):
            T.distance_texture(m, bad)
    with pytest.raises(ValueError):
        T.distance_texture(m, edt='bogus')
    pic = m.astype(np.uint8) * 255
    pytest.importorskip('PIL')
    import sdf_amd
    with pytest.raises(ValueError):
        sdf_amd.image(pic, edt='bogus')
    font = ref.dejavu()
    if font is not None:
        with pytest.raises(ValueError):
            sdf_amd.text(font, 'Hi', points=32, edt='bogus')


def test_abi_has_the_entry_point():
    assert 'sdf_distance_texture_host' in engine.ABI and engine.ABI_VERSION >= 12
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_distance_texture_host\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == engine.ABI_VERSION
    assert callable(getattr(engine.Engine, 'distance_texture'))


def test_entry_point_refuses_null_arguments_without_a_device():
    lib = engine.load_library()
    buf = np.zeros(4, np.uint8)
    out = np.zeros(4, np.float64)
    p8, p64 = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.sdf_distance_texture_host(None, p8, 2, 2, p64) == 2
    assert b'sdf_distance_texture_host' in lib.sdf_last_error()


NO_SCIPY = r'''
import importlib, sys
sys.modules['scipy'] = None                      # any `import scipy...` now raises ImportError
sys.modules['scipy.ndimage'] = None
import numpy as np
import sdf_amd
from sdf_amd import engine, tape
import edt_ref
T = importlib.import_module('sdf_amd.text')
seen = []
class FakeEngine:                                # the engine is where the device begins: stand in for it
    def distance_texture(self, mask):
        seen.append(np.array(mask, dtype=bool))
        return edt_ref.distance_texture(mask)
engine.get_engine = lambda *a, **k: FakeEngine()
pic = edt_ref.cases()['frame'].astype(np.uint8) * 255
try:
    sdf_amd.image(pic, width=3.0)
    raise SystemExit('the host path ran without scipy: the block does not work')
except ImportError:
    pass
f = sdf_amd.image(pic, width=3.0, edt='device')
T.EDT = 'device'
g = sdf_amd.image(pic, width=3.0)
assert len(seen) == 2 and np.array_equal(seen[0], edt_ref.cases()['frame']) and np.array_equal(seen[1], seen[0])
a, b = tape.lower(f), tape.lower(g)
assert np.array_equal(a.consts.view(np.int64), b.consts.view(np.int64)) and len(a.consts) > pic.size
font = edt_ref.dejavu()
if font is not None:
    sdf_amd.text(font, 'Hi', points=32)
    assert len(seen) == 3 and seen[2].any() and not seen[2].all()
assert sys.modules['scipy'] is None and not [m for m in sys.modules if m.startswith('scipy.') and sys.modules[m] is not None]
print('ok', len(seen))
'''


def test_device_mode_does_not_import_scipy():
    pytest.importorskip('PIL')
    script = 'import sys\nsys.path[:0] = [%r, %r]\n' % (ROOT, os.path.join(ROOT, 'tests')) + NO_SCIPY
    r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith('ok'), r.stdout + r.stderr
