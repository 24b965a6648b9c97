"""Indexed mesh files without meshio: binary little-endian PLY and Wavefront OBJ of a welded mesh, optionally with the
field's normals at the vertices.  `save` comes here for `.ply` / `.obj` when `normals=True`,
`writer='native'`, or meshio does not import.

The PLY body is packed on the device (`engine.Mesh.ply_records`: k_ply_vertices / k_ply_faces) and written with one header;
OBJ is text and is formatted here, on the host -- it is not the fast path.  Both carry the float32 cast of the float64
vertices: `%.9g` round-trips a float32, so a model saved either way holds the same numbers.  tests/normals_ref.py restates the
layouts and the normal's definition; nothing here imports meshio."""
import os

import numpy as np

NATIVE_EXTENSIONS = ('.ply', '.obj')


def ply_header(n_vertices, n_faces, with_normals, quality=None):
    """the header of a binary little-endian PLY file of n_vertices float32 vertices (with float32 normals; with quality, a float32
    scalar per vertex after them under MeshLab's name, `property float quality`) and n_faces triangles"""
    lines = ['ply', 'format binary_little_endian 1.0', 'comment sdf_amd', 'element vertex %d' % n_vertices,
             'property float x', 'property float y', 'property float z']
    if with_normals:
        lines += ['property float nx', 'property float ny', 'property float nz']
    if quality is not None and quality is not False:
        lines += ['property float quality']
    lines += ['element face %d' % n_faces, 'property list uchar int vertex_indices', 'end_header']
    return ('\n'.join(lines) + '\n').encode('ascii')


def ply_records(points, cells, normals=None, quality=None):
    """(vertex_bytes, face_bytes) of a host mesh: what `engine.Mesh.ply_records` packs on the device; quality: a scalar per vertex,
    appended to each vertex record as a float32 (inf and nan as they are)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = np.asarray(cells).reshape(-1, 3)
    if len(points) >= 1 << 31:
        raise ValueError('%d vertices: the face records hold 32-bit indices' % len(points))
    cols = [points.astype('<f4')]
    if normals is not None:
        cols.append(np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype('<f4'))
    if quality is not None:
        q = np.asarray(quality, dtype=np.float64).reshape(-1, 1)
        if len(q) != len(points):
            raise ValueError('%d quality values for %d vertices' % (len(q), len(points)))
        with np.errstate(over='ignore'):
            cols.append(q.astype('<f4'))
    vertex = np.ascontiguousarray(np.hstack(cols)).view(np.uint8).reshape(-1)
    face = np.empty(len(cells), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    face['n'] = 3
    face['v'] = cells
    return vertex, face.view(np.uint8).reshape(-1)


def write_ply(path, vertex_bytes, face_bytes, n_vertices, n_faces, with_normals, quality=None):
    """header + the two record blocks, as they come from the device (quality: the vertex records end in a float32 scalar)"""
    quality = quality is not None and quality is not False
    vertex_bytes = np.ascontiguousarray(vertex_bytes, dtype=np.uint8).reshape(-1)
    face_bytes = np.ascontiguousarray(face_bytes, dtype=np.uint8).reshape(-1)
    if len(vertex_bytes) != n_vertices * ((24 if with_normals else 12) + (4 if quality else 0)) or len(face_bytes) != n_faces * 13:
        raise ValueError('%d vertex bytes and %d face bytes do not hold %d vertices%s%s and %d faces'
                         % (len(vertex_bytes), len(face_bytes), n_vertices, ' with normals' if with_normals else '',
                            ' with quality' if quality else '', n_faces))
    with open(path, 'wb') as fp:
        fp.write(ply_header(n_vertices, n_faces, with_normals, quality or None))
        fp.write(memoryview(vertex_bytes))
        fp.write(memoryview(face_bytes))


def write_obj(path, points, cells, normals=None):
    """`v x y z` per vertex (%.9g of the float32 cast), `vn` per vertex and `f a//a b//b c//c` when normals are given, else
    `f a b c`; indices are 1-based"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)
    c = np.asarray(cells).reshape(-1, 3).astype(np.int64) + 1
    with open(path, 'w', newline='\n') as fp:
        fp.write('# sdf_amd\n')
        fp.write(''.join(['v %.9g %.9g %.9g\n' % (x, y, z) for x, y, z in p.tolist()]))
        if normals is not None:
            n = np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)
            fp.write(''.join(['vn %.9g %.9g %.9g\n' % (x, y, z) for x, y, z in n.tolist()]))
            fp.write(''.join(['f %d//%d %d//%d %d//%d\n' % (a, a, b, b, d, d) for a, b, d in c.tolist()]))
        else:
            fp.write(''.join(['f %d %d %d\n' % (a, b, d) for a, b, d in c.tolist()]))


def frozen(a, dtype=None):
    """a read-only copy of `a` (as `dtype`, if given): what the result objects of the package hand out"""
    a = np.array(a, dtype=dtype)
    a.setflags(write=False)
    return a


def central_difference(f, P, eps):
    """g (N, 3) float64, the host definition of the probes' central difference over f(Q) -> (N,) float64 at the points P (N, 3)
    float64: for axis k the value at x_k + eps minus the value at x_k + (-eps), plus taken first -- one rounding per operation,
    what the device kernels reproduce bit for bit (csrc/sdf_probe.h)"""
    g = np.empty((len(P), 3))
    for k in range(3):
        Q = P.copy()
        Q[:, k] = P[:, k] + eps
        plus = f(Q)
        Q[:, k] = P[:, k] + (-eps)
        minus = f(Q)
        g[:, k] = plus - minus
    return g


def vertex_normals(ev, points, eps):
    """the normal's definition on the host over an evaluator ev(P) -> (N,) float64: where the device kernel does not reach (a
    model with user closures, a soup gathered on the host).  float64, one rounding per operation: for axis k the value at
    x_k + eps minus the value at x_k + (-eps), len = sqrt((g0*g0 + g1*g1) + g2*g2), n = g / len; a vertex whose len is 0 or
    NaN is flat -- normal (0, 0, 0), counted.  Returns (normals (U, 3), n_flat)."""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    eps = float(eps)
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError('eps must be finite and positive, got %r' % eps)
    if len(P) == 0:
        return np.zeros((0, 3)), 0
    g = central_difference(lambda Q: np.asarray(ev(Q), dtype=np.float64).reshape(-1), P, eps)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    flat = (ln == 0) | np.isnan(ln)
    with np.errstate(invalid='ignore', divide='ignore'):
        n = g / ln[:, None]
    n[flat] = 0.0
    return n, int(flat.sum())


def _has_meshio():
    try:
        import meshio  # noqa: F401
        return True
    except ImportError:
        return False


def choose_writer(path, writer=None, normals=False, thickness=False, curvature=False):
    """which writer `save` uses for `path`: 'stl', 'meshio' or 'native'.  writer=None: native when normals are asked for,
    else meshio where it imports (as before there was a native writer), else native for .ply / .obj.  Raises ValueError for
    what no writer serves (vertex normals in an STL file or through meshio, a native extension other than .ply / .obj, an
    unknown writer) and ImportError where only meshio could serve and it is not installed.  thickness: the file is to carry the
    wall thickness per vertex -- .ply and the native writer only, anything else raises ValueError.  curvature: it is to carry a
    curvature per vertex, through the same door; a file has one `quality` column, so both together raise ValueError."""
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if writer not in (None, 'native', 'meshio'):
        raise ValueError("writer must be None, 'native' or 'meshio', got %r" % (writer,))
    if thickness and curvature:
        raise ValueError('a .ply file has one `quality` property: give thickness= or curvature=, not both')
    if thickness or curvature:
        what = 'wall thickness' if thickness else 'curvature'
        if ext != '.ply':
            raise ValueError("the %s is written as a .ply file's `quality` property, not into %r" % (what, ext))
        if writer == 'meshio':
            raise ValueError("the meshio writer does not write the %s: use writer='native'" % what)
        return 'native'
    if ext == '.stl':
        if normals:
            raise ValueError('STL has no vertex normals: save a .ply or an .obj with normals=True')
        return 'stl'
    if writer == 'meshio':
        if normals:
            raise ValueError("the meshio writer does not write the field's normals: use writer='native'")
        return 'meshio'
    if writer is None and not normals and _has_meshio():
        return 'meshio'
    if ext in NATIVE_EXTENSIONS:
        return 'native'
    if writer is None and not normals:
        import meshio  # noqa: F401  (not installed: the ImportError a save of this extension always raised)
    raise ValueError('the native writer serves %s and %s, not %r' % (NATIVE_EXTENSIONS + (ext,)))
