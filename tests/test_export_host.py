"""The definition of the indexed export (tests/normals_ref.py) over the CPU checker, and the host side of the PLY / OBJ writers: the
ABI entries, the record layouts, the files, which writer `save` picks, and that the native path never imports meshio.  No GPU."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import normals_ref as ref
from sdf_amd import core, dist, engine, meshfile, stl
from sdf_amd.measure import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a hand-made mesh: 4 vertices, 2 triangles; values that are not float32 numbers, a negative zero, a large and a tiny one
PTS = np.array([[0.1, -0.2, 0.3], [1.0 / 3.0, 2.0 ** -30, -0.0], [1e6 + 0.015625, -7.25, 3.0], [0.7, 0.7, -123456.789]])
CELLS = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
NRM = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [1.0 / 3.0, 2.0 / 3.0, -2.0 / 3.0], [0.0, 0.0, 0.0]])
_sphere = {}


def sphere_mesh(ns, oracle):
    """the welded `oracle.generate` mesh of sphere(1), bounds +-1.1, samples 2^13, and its normals by the definition at
    eps = 1e-3 over the CPU checker: computed once"""
    if not _sphere:
        f = ns['sphere'](1)
        X, Y, Z, _ = core.grid_axes(((-1.1, -1.1, -1.1), (1.1, 1.1, 1.1)), samples=2 ** 13)
        soup = oracle.generate(f, X, Y, Z, 32, True).points
        pts, inv = np.unique(soup, axis=0, return_inverse=True)
        cells = np.asarray(inv).reshape(-1, 3)
        n, n_flat = ref.vertex_normals(lambda P: oracle.evaluate(f, P), pts, 1e-3)
        for a in (pts, cells, n):
            a.setflags(write=False)
        _sphere.update(f=f, pts=pts, cells=cells, n=n, n_flat=n_flat)
    return _sphere


def test_abi_has_the_entry_points():
    assert 'sdf_mesh_vertex_normals' in engine.ABI and 'sdf_mesh_emit_ply_host' in engine.ABI and engine.ABI_VERSION >= 14
    assert 'sdf_mesh_normals_last_kernel_ms' in engine.ABI
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_mesh_vertex_normals\s*\(', hdr) and re.search(r'\bint\s+sdf_mesh_emit_ply_host\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == engine.ABI_VERSION
    assert callable(getattr(engine.Mesh, 'vertex_normals')) and callable(getattr(engine.Mesh, 'ply_records'))


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = engine.load_library()
    flat = ctypes.c_int64(0)
    assert lib.sdf_mesh_vertex_normals(None, None, 1e-3, None, ctypes.byref(flat)) == 2
    assert b'sdf_mesh_vertex_normals' in lib.sdf_last_error()
    assert lib.sdf_mesh_emit_ply_host(None, 0, None, None) == 2
    assert b'sdf_mesh_emit_ply_host' in lib.sdf_last_error()


def test_sphere_mesh_is_the_one_the_bounds_were_worked_out_on(ns, oracle_lib):
    m = sphere_mesh(ns, oracle_lib)
    assert len(m['cells']) == 3200 and len(m['pts']) == 1602 and m['n_flat'] == 0


def test_definition_gives_unit_normals(ns, oracle_lib):
    n = sphere_mesh(ns, oracle_lib)['n']
    ln = np.sqrt((n ** 2).sum(axis=1))
    assert (np.abs(ln - 1) <= 4 * np.spacing(1.0)).all(), np.abs(ln - 1).max()


def test_definition_on_a_sphere_is_the_radial_direction(ns, oracle_lib):
    m = sphere_mesh(ns, oracle_lib)
    p = m['pts']
    r = np.sqrt((p ** 2).sum(axis=1))
    err = np.abs(m['n'] - p / r[:, None]).max()
    print('largest deviation of a normal from p / |p| at eps = 1e-3: %.3g' % err)
    assert err <= 1e-6                  # the truncation term of the central difference is of order eps^2


def test_normals_point_the_way_the_faces_wind(ns, oracle_lib):
    m = sphere_mesh(ns, oracle_lib)
    p, c, n = m['pts'], m['cells'], m['n']
    a, b, d = p[c[:, 0]], p[c[:, 1]], p[c[:, 2]]
    fn = np.cross(b - a, d - a)
    assert ((fn * (a + b + d)).sum(axis=1) > 0).all()                       # away from the centre
    fn = fn / np.sqrt((fn ** 2).sum(axis=1))[:, None]
    dots = np.stack([(fn * n[c[:, q]]).sum(axis=1) for q in range(3)])
    print('smallest face . vertex normal: %.4f' % dots.min())
    assert dots.min() > 0.9


def test_a_vertex_without_a_gradient_is_flat(ns, oracle_lib):
    f = sphere_mesh(ns, oracle_lib)['f']
    P = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, -2.0, 0.0]])
    n, n_flat = ref.vertex_normals(lambda Q: oracle_lib.evaluate(f, Q), P, 1e-3)
    assert n_flat == 1 and not n[0].any() and np.array_equal(np.signbit(n[0]), [False] * 3)
    assert np.allclose(n[1], [1, 0, 0], atol=1e-6) and np.allclose(n[2], [0, -1, 0], atol=1e-6)
    # NaN counts as flat too
    n, n_flat = ref.vertex_normals(lambda Q: np.where(Q[:, 0] > 0.4, np.nan, oracle_lib.evaluate(f, Q).reshape(-1)), P, 1e-3)
    assert n_flat == 2 and not n[:2].any()
    n, n_flat = ref.vertex_normals(lambda Q: 1 / 0, np.zeros((0, 3)), 1e-3)
    assert n.shape == (0, 3) and n_flat == 0


def test_package_restatement_equals_the_definition(ns, oracle_lib):
    m = sphere_mesh(ns, oracle_lib)
    ev = lambda P: oracle_lib.evaluate(m['f'], P)
    P = np.vstack([m['pts'][::7], np.zeros((1, 3))])
    a, fa = ref.vertex_normals(ev, P, 1e-3)
    b, fb = meshfile.vertex_normals(ev, P, 1e-3)
    assert fa == fb == 1 and np.array_equal(a.view(np.int64), b.view(np.int64))
    for bad in (0.0, -1e-3, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            meshfile.vertex_normals(ev, P, bad)


@pytest.mark.parametrize('with_normals', (False, True))
def test_ply_records_and_header(with_normals):
    nrm = NRM if with_normals else None
    vb, fb = ref.ply_records(PTS, CELLS, nrm)
    assert vb.dtype == np.uint8 and len(vb) == 4 * (24 if with_normals else 12) and len(fb) == 2 * 13
    v = vb.view('<f4').reshape(4, -1)
    assert np.array_equal(v[:, :3].view(np.int32), PTS.astype(np.float32).view(np.int32))
    if with_normals:
        assert np.array_equal(v[:, 3:].view(np.int32), NRM.astype(np.float32).view(np.int32))
    assert bytes(fb[:13]) == b'\x03' + b'\x00\x00\x00\x00' + b'\x01\x00\x00\x00' + b'\x02\x00\x00\x00'
    assert bytes(fb[13:]) == b'\x03' + b'\x02\x00\x00\x00' + b'\x01\x00\x00\x00' + b'\x03\x00\x00\x00'
    pv, pf = meshfile.ply_records(PTS, CELLS, nrm)
    assert np.array_equal(pv, vb) and np.array_equal(pf, fb)
    want = ['ply', 'format binary_little_endian 1.0', 'comment sdf_amd', 'element vertex 4', 'property float x', 'property float y',
            'property float z'] + (['property float nx', 'property float ny', 'property float nz'] if with_normals else []) + \
           ['element face 2', 'property list uchar int vertex_indices', 'end_header']
    assert ref.ply_header(4, 2, with_normals) == ('\n'.join(want) + '\n').encode()
    assert meshfile.ply_header(4, 2, with_normals) == ref.ply_header(4, 2, with_normals)


@pytest.mark.parametrize('with_normals', (False, True))
def test_write_ply_round_trip(tmp_path, with_normals):
    nrm = NRM if with_normals else None
    vb, fb = ref.ply_records(PTS, CELLS, nrm)
    path = str(tmp_path / 'a.ply')
    meshfile.write_ply(path, vb, fb, 4, 2, with_normals)
    assert os.path.getsize(path) == len(ref.ply_header(4, 2, with_normals)) + 4 * (24 if with_normals else 12) + 2 * 13
    p, n, c, head = ref.parse_ply(path)
    assert head == ref.ply_header(4, 2, with_normals)
    assert np.array_equal(p.view(np.int32), PTS.astype(np.float32).view(np.int32)) and np.array_equal(c, CELLS)
    assert (n is None) if not with_normals else np.array_equal(n.view(np.int32), NRM.astype(np.float32).view(np.int32))
    with pytest.raises(ValueError):
        meshfile.write_ply(path, vb[:-1], fb, 4, 2, with_normals)
    with pytest.raises(ValueError):
        meshfile.write_ply(path, vb, fb, 4, 2, not with_normals)


@pytest.mark.parametrize('with_normals', (False, True))
def test_write_obj_round_trip(tmp_path, with_normals):
    nrm = NRM if with_normals else None
    path = str(tmp_path / 'a.obj')
    meshfile.write_obj(path, PTS, CELLS, nrm)
    lines = [l for l in open(path).read().split('\n') if l and not l.startswith('#')]
    assert lines == ref.obj_lines(PTS, CELLS, nrm)
    assert lines[-1] == ('f 3//3 2//2 4//4' if with_normals else 'f 3 2 4')
    p, n, c = ref.parse_obj(path)
    # %.9g round-trips a float32: the text holds the PLY file's numbers (the sign of a zero included)
    assert np.array_equal(p.view(np.int32), PTS.astype(np.float32).view(np.int32)) and np.array_equal(c, CELLS)
    assert (n is None) if not with_normals else np.array_equal(n.view(np.int32), NRM.astype(np.float32).view(np.int32))


class _FakeMeshio:
    pass


@pytest.mark.parametrize('have_meshio', (False, True))
def test_writer_selection(monkeypatch, have_meshio):
    monkeypatch.setitem(sys.modules, 'meshio', _FakeMeshio() if have_meshio else None)
    for ext, writer, normals in itertools.product(('.stl', '.ply', '.obj', '.off', '.PLY'), (None, 'native', 'meshio'), (False, True)):
        cell = (ext, writer, normals, have_meshio)
        pick = lambda: meshfile.choose_writer('dir.v2/a' + ext, writer, normals)
        native_ext = ext.lower() in ('.ply', '.obj')
        if ext == '.stl':
            if normals:
                with pytest.raises(ValueError, match='STL has no vertex normals'):
                    pick()
            else:
                assert pick() == 'stl', cell
        elif writer == 'meshio':
            if normals:
                with pytest.raises(ValueError, match='meshio'):
                    pick()
            else:
                assert pick() == 'meshio', cell               # today's path: `import meshio` raises there when it is absent
        elif writer == 'native' or normals:
            if native_ext:
                assert pick() == 'native', cell
            else:
                with pytest.raises(ValueError, match=r'\.ply and \.obj'):
                    pick()
        elif have_meshio:
            assert pick() == 'meshio', cell                   # the default where meshio is installed does not change
        elif native_ext:
            assert pick() == 'native', cell
        else:
            with pytest.raises(ImportError):
                pick()
    with pytest.raises(ValueError, match='writer'):
        meshfile.choose_writer('a.ply', 'trimesh', False)


NO_MESHIO = r'''
import contextlib, importlib, importlib.abc, sys, types
asked = []
class Watch(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path=None, target=None):
        if name == 'meshio' or name.startswith('meshio.'):
            asked.append(name)
        return None
sys.meta_path.insert(0, Watch())
import numpy as np
import sdf_amd
from sdf_amd import core
import normals_ref as ref
T = importlib.import_module(sys.argv[2])          # this test module: PTS, CELLS, NRM
TAPE = types.SimpleNamespace(tape=types.SimpleNamespace(externs=[]))
BOUNDS = ((-1.0, -2.0, -3.0), (3.0, 1.0, 9.0))    # its diagonal is 13
DEFAULT_EPS = 1e-4 * 6.5
class StubMesh:
    # a device mesh that holds T.PTS / T.CELLS and notes what is asked of it
    def __init__(self):
        self.log = []
    @property
    def n_triangles(self):
        self.log.append('n_triangles')
        return len(T.CELLS)
    def weld(self):
        self.log.append('weld')
        return T.PTS, T.CELLS
    def vertex_normals(self, tape, eps):
        self.log.append(('vertex_normals', tape, eps))
        return T.NRM, 1
    def ply_records(self, normals=False):
        self.log.append(('ply_records', normals))
        return ref.ply_records(T.PTS, T.CELLS, T.NRM if normals else None)
calls = []
@contextlib.contextmanager
def fake_meshed(sdf, *args, keep=None, to_host=False, **kw):          # `meshed` is where the device begins: stand in for it
    mesh = StubMesh()
    calls.append((mesh.log, args, keep, to_host, kw))
    yield core.Meshed(mesh, None, TAPE, None, BOUNDS, {})
core.meshed = fake_meshed
f = sdf_amd.sphere(1)
try:
    f.save(sys.argv[1] + '/a.stl', normals=True)
    raise SystemExit('an STL file with vertex normals was not refused')
except ValueError as e:
    assert 'STL has no vertex normals' in str(e)
assert not calls
for name, kw in (('n.ply', dict(normals=True)), ('p.ply', dict(writer='native')), ('n.obj', dict(normals=True, normal_eps=0.5)),
                 ('p.obj', dict(writer='native', samples=64))):
    f.save(sys.argv[1] + '/' + name, **kw)
# normals taken or not and with which step; the PLY body packed by the mesh, the OBJ's weld fetched
assert [c[0] for c in calls] == [[('vertex_normals', TAPE, DEFAULT_EPS), ('ply_records', True), 'n_triangles'],
                                 [('ply_records', False), 'n_triangles'],
                                 [('vertex_normals', TAPE, 0.5), 'weld'],
                                 ['weld']], calls
assert [c[1:] for c in calls] == [((), None, False, {})] * 3 + [((), None, False, {'samples': 64})], calls
for name, wn in (('n.ply', True), ('p.ply', False)):
    p, n, c, head = ref.parse_ply(sys.argv[1] + '/' + name)
    assert np.array_equal(p, T.PTS.astype(np.float32)) and np.array_equal(c, T.CELLS) and (n is not None) == wn
for name, wn in (('n.obj', True), ('p.obj', False)):
    p, n, c = ref.parse_obj(sys.argv[1] + '/' + name)
    assert np.array_equal(p, T.PTS.astype(np.float32)) and np.array_equal(c, T.CELLS) and (n is not None) == wn
pts, cells, nrm = f.generate_mesh(normals=True, samples=64)
assert pts is T.PTS and cells is T.CELLS and nrm is T.NRM and core.generate_mesh.last_flat == 1
assert calls[-1] == ([('vertex_normals', TAPE, DEFAULT_EPS), 'weld'], (), None, False, {'samples': 64}), calls[-1]
assert not asked and 'meshio' not in sys.modules, asked
# the default writer keeps meshio where it is installed and, without it, writes the native file
sys.modules['meshio'] = None
f.save(sys.argv[1] + '/d.ply')
assert calls[-1][0] == [('ply_records', False), 'n_triangles'] and ref.parse_ply(sys.argv[1] + '/d.ply')[1] is None
print('ok', len(calls))
'''


def test_native_path_never_imports_meshio(tmp_path):
    script = 'import sys\nsys.path[:0] = [%r, %r]\n' % (ROOT, os.path.join(ROOT, 'tests')) + NO_MESHIO
    r = subprocess.run([sys.executable, '-c', script, str(tmp_path), __name__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith('ok'), r.stdout + r.stderr


# ---- a multi-process run whose soup was gathered on the host: `core.meshed` yields no device mesh and every reader says what it does then ----
SOUP = PTS[CELLS].reshape(-1, 3)          # two triangles, six rows, four distinct points
BOUNDS = ((-1.0, -2.0, -3.0), (3.0, 1.0, 9.0))          # its diagonal is 13
STATS = {'skipped': 3, 'empty': 4, 'nonempty': 1}


class StubEngine:
    precision = engine.PRECISION_F64

    def tape_for(self, sdf):
        return ('tape of', sdf)

    def eval_points(self, tape, P):
        assert tape == ('tape of', 'model')
        return np.sqrt((np.asarray(P) ** 2).sum(axis=1)) - 1.0


@pytest.fixture
def gathered(monkeypatch):
    """a world of two ranks whose exchange hands back the soup in HOST memory; the list counts the engines asked for"""
    import torch
    asked = []
    monkeypatch.setattr(dist, 'world_size', lambda: 2)
    monkeypatch.setattr(dist, 'generate_sharded_device', lambda eng, tape, X, Y, Z, batch_size, sparse: (torch.from_numpy(SOUP.reshape(-1).copy()), STATS))
    monkeypatch.setattr(engine, 'get_engine', lambda device=None: asked.append(device) or StubEngine())
    return asked


def test_host_gathered_soup_is_read_on_the_host(gathered, monkeypatch, tmp_path, capsys):
    got = core.generate('model', bounds=BOUNDS, samples=64, workers=5)
    assert got.dtype == np.float64 and np.array_equal(got, SOUP) and core.generate.last_stats is STATS
    out = capsys.readouterr().out.split('\n')
    assert out[0] == 'min -1, -2, -3' and out[1] == 'max 3, 1, 9' and out[2].startswith('step ') and out[3].endswith('with 5 workers')
    assert out[4] == '3 skipped, 4 empty, 1 nonempty' and out[5].startswith('2 triangles in ')

    core.save(str(tmp_path / 'x.stl'), 'model', bounds=BOUNDS, samples=64, verbose=False)
    stl.write_binary_stl(str(tmp_path / 'want.stl'), SOUP)
    assert (tmp_path / 'x.stl').read_bytes() == (tmp_path / 'want.stl').read_bytes()

    wp, wc = np.unique(SOUP, axis=0, return_inverse=True)
    wc = np.asarray(wc).reshape(-1, 3)
    pts, cells, nrm = core.generate_mesh('model', bounds=BOUNDS, samples=64, verbose=False)
    assert nrm is None and np.array_equal(pts, wp) and np.array_equal(cells, wc) and len(pts) == 4 and cells.shape == (2, 3)

    seen = []
    real = meshfile.vertex_normals
    monkeypatch.setattr(meshfile, 'vertex_normals', lambda ev, P, eps: seen.append((P, eps)) or real(ev, P, eps))
    pts, cells, nrm = core.generate_mesh('model', normals=True, bounds=BOUNDS, samples=64, verbose=False)
    assert len(seen) == 1 and np.array_equal(seen[0][0], wp) and seen[0][1] == 1e-4 * 6.5
    want, flat = real(lambda P: StubEngine().eval_points(('tape of', 'model'), P), wp, 1e-4 * 6.5)
    assert np.array_equal(nrm, want) and core.generate_mesh.last_flat == flat and np.array_equal(pts, wp) and np.array_equal(cells, wc)
    core.save(str(tmp_path / 'n.ply'), 'model', normals=True, normal_eps=0.5, bounds=BOUNDS, samples=64, verbose=False)
    assert seen[-1][1] == 0.5 and (tmp_path / 'n.ply').read_bytes().endswith(b''.join(a.tobytes() for a in meshfile.ply_records(wp, wc, real(
        lambda P: StubEngine().eval_points(('tape of', 'model'), P), wp, 0.5)[0])))


def test_host_gathered_soup_cannot_be_measured_or_split(gathered, tmp_path):
    with pytest.raises(NotImplementedError, match='measure: the soup of this multi-process run was gathered on the host'):
        measure('model', bounds=BOUNDS, samples=64, verbose=False)
    for call in (lambda: core.generate_mesh('model', keep='largest', bounds=BOUNDS, samples=64, verbose=False),
                 lambda: core.save(str(tmp_path / 'k.stl'), 'model', keep=1, bounds=BOUNDS, samples=64, verbose=False),
                 lambda: core.save(str(tmp_path / 'k.ply'), 'model', keep=[True], writer='native', bounds=BOUNDS, samples=64, verbose=False),
                 lambda: measure('model', keep=lambda sh: sh.triangles > 1, bounds=BOUNDS, samples=64, verbose=False)):
        with pytest.raises(NotImplementedError, match='keep: the soup of this multi-process run was gathered on the host'):
            call()
    assert not (tmp_path / 'k.stl').exists() and not (tmp_path / 'k.ply').exists()
    # a keep that no mesh could satisfy is still refused first: no engine is asked for
    del gathered[:]
    for call in (lambda: core.generate_mesh('model', keep='smallest', bounds=BOUNDS), lambda: measure('model', keep=-3, bounds=BOUNDS),
                 lambda: core.save(str(tmp_path / 'k.stl'), 'model', keep=2.5, bounds=BOUNDS)):
        with pytest.raises(ValueError, match='keep'):
            call()
    assert gathered == []
