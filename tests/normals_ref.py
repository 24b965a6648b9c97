"""The definition of the indexed export: the field's normal at a vertex, the binary PLY records and header,
the OBJ text.  NumPy over an evaluator `ev(P) -> (N,) float64`; csrc/sdf_normals.hip (k_vertex_normals) and csrc/sdf_plain.hip
(k_ply_vertices, k_ply_faces) reproduce it bit for bit, sdf_amd/meshfile.py byte for byte.

Everything is float64 with one rounding per written operation.  The order is that of k_render's normal phase: for each axis the
value at +eps first, then at -eps, g = v_plus - v_minus."""
import numpy as np


def vertex_normals(ev, points, eps):
    """(normals (U, 3) float64, n_flat) at points (U, 3) float64"""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    eps = np.float64(eps)
    U = len(P)
    g = np.zeros((U, 3), np.float64)
    for k in range(3):
        plus = P.copy()
        plus[:, k] = P[:, k] + eps                 # only coordinate k changes
        minus = P.copy()
        minus[:, k] = P[:, k] + (-eps)
        v_plus = np.asarray(ev(plus), dtype=np.float64).reshape(-1) if U else np.zeros(0)
        v_minus = np.asarray(ev(minus), dtype=np.float64).reshape(-1) if U else np.zeros(0)
        g[:, k] = v_plus - v_minus
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ln = np.sqrt((g0 * g0 + g1 * g1) + g2 * g2)
        flat = (ln == 0) | (ln != ln)
        n = g / ln[:, None]
    n[flat] = 0.0
    return n, int(flat.sum())


def ply_records(points, cells, normals=None):
    """(vertex_bytes, face_bytes) uint8: float32 x, y, z (+ float32 nx, ny, nz) per vertex; uint8 3 + 3 x int32 per face"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    C = np.asarray(cells).reshape(-1, 3)
    rec = P.astype('<f4')
    if normals is not None:
        rec = np.concatenate([rec, np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype('<f4')], axis=1)
    vertex = np.frombuffer(np.ascontiguousarray(rec).tobytes(), np.uint8)
    face = bytearray()
    for a, b, c in C.tolist():
        face += b'\x03' + int(a).to_bytes(4, 'little', signed=True) + int(b).to_bytes(4, 'little', signed=True) + int(c).to_bytes(4, 'little', signed=True)
    return vertex, np.frombuffer(bytes(face), np.uint8)


def ply_header(U, T, with_normals):
    lines = ['ply', 'format binary_little_endian 1.0', 'comment sdf_amd', 'element vertex %d' % U, 'property float x', 'property float y',
             'property float z']
    if with_normals:
        lines += ['property float nx', 'property float ny', 'property float nz']
    lines += ['element face %d' % T, 'property list uchar int vertex_indices', 'end_header']
    return ''.join(l + '\n' for l in lines).encode('ascii')


def obj_lines(points, cells, normals=None):
    """the lines of the OBJ file that carry data (comments aside): v, then vn, then f"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    out = ['v %.9g %.9g %.9g' % (float(x), float(y), float(z)) for x, y, z in P]
    C = np.asarray(cells).reshape(-1, 3)
    if normals is None:
        return out + ['f %d %d %d' % (a + 1, b + 1, c + 1) for a, b, c in C.tolist()]
    N = np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    out += ['vn %.9g %.9g %.9g' % (float(x), float(y), float(z)) for x, y, z in N]
    return out + ['f %d//%d %d//%d %d//%d' % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in C.tolist()]


def parse_ply(path):
    """(points float32 (U, 3), normals float32 (U, 3) or None, cells int32 (T, 3), header bytes) of a file this project writes"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    head = raw[:end].decode('ascii').split('\n')
    U = int([l for l in head if l.startswith('element vertex')][0].split()[-1])
    T = int([l for l in head if l.startswith('element face')][0].split()[-1])
    w = 6 if 'property float nx' in head else 3
    assert len(raw) == end + U * 4 * w + T * 13, (len(raw), end, U, T, w)
    v = np.frombuffer(raw, '<f4', U * w, end).reshape(U, w)
    f = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), T, end + U * 4 * w)
    assert (f['n'] == 3).all()
    return v[:, :3], (v[:, 3:] if w == 6 else None), f['v'], raw[:end]


def parse_obj(path):
    """(points float32, normals float32 or None, cells int64 0-based) of a file this project writes"""
    v, vn, f = [], [], []
    for line in open(path):
        t = line.split()
        if not t or t[0].startswith('#'):
            continue
        if t[0] == 'v':
            v.append([float(x) for x in t[1:]])
        elif t[0] == 'vn':
            vn.append([float(x) for x in t[1:]])
        elif t[0] == 'f':
            idx = [x.split('//') for x in t[1:]]
            assert all(len(set(i)) == 1 for i in idx), line       # a//a: the normal's index is the vertex's
            f.append([int(i[0]) - 1 for i in idx])
        else:
            raise AssertionError('unexpected OBJ line: %r' % line)
    P = np.array(v, np.float64).reshape(-1, 3).astype(np.float32)
    N = np.array(vn, np.float64).reshape(-1, 3).astype(np.float32) if vn else None
    return P, N, np.array(f, np.int64).reshape(-1, 3)
