"""Triangle mesh -> SDF leaf (reference sdf/mesh.py:8-113).

The reference voxelises a mesh with OpenVDB into a narrow-band level set, copies the active voxels
into a dense float32 array and evaluates it with scipy's RegularGridInterpolator, falling back to
the distance to the bounding box beyond the band (reference sdf/mesh.py:64-113).  Here the lookup
is the `grid3d` leaf of the op tape: the voxel array and its three axes travel to the device with
the tape's constants and the interpreter does the trilinear interpolation per sample
(csrc/sdf_interp.h L_GRID3D, same operation order as scipy 1.7.1's `_evaluate_linear`).

`grid_sdf` builds the leaf from a ready voxel grid (any producer); `Mesh.sdf` is the reference's
entry point and needs `pyopenvdb` for the voxelisation step only -- without it the import fails
exactly where the reference's does (reference sdf/mesh.py:66).  `level_set` (`Mesh.sdf(...,
voxelizer='device')`) makes the grid on the device instead (csrc/sdf_level_set.hip, DESIGN.md
section 4c); `Mesh.from_stl` reads a binary STL without meshio.
"""
import numpy as np

from .d3 import SDF3, box
from .ir import Node, unwrap


def grid_sdf(xyz, array, background, bounding_box):
    """the SDF3 the reference's `Mesh.sdf` returns, from its ingredients (reference sdf/mesh.py:88-105):
    `xyz` the three strictly increasing coordinate axes of the voxel centres, `array` the float32
    voxel values of shape (len(X), len(Y), len(Z)), `background` the narrow-band value
    (`grid.background`), `bounding_box` = (a, b) of the mesh for the `box(a=a, b=b)` estimator."""
    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in xyz)
    A = np.ascontiguousarray(array, dtype=np.float32)          # scipy keeps float32 values as they are
    if A.shape != (len(X), len(Y), len(Z)):
        raise ValueError('There are %d points and %d values in dimension 0' % (len(X), A.shape[0] if A.ndim else 0))
    for i, g in enumerate((X, Y, Z)):
        if len(g) < 2 or not np.all(np.diff(g) > 0):
            raise ValueError('The points in dimension %d must be strictly ascending' % i)
    a, b = bounding_box
    est = unwrap(box(a=a, b=b))                                # Node('box', centre + half size): d3.py:122-134
    params = [len(X), len(Y), len(Z), float(background)] + list(est.params)
    blob = np.concatenate([X, Y, Z, A.astype(np.float64).reshape(-1)])
    f = SDF3(Node('grid3d', params, (), meta={'blob': blob}))
    f.array, f.xyz = A, (X, Y, Z)                              # what the reference hangs on its closure (mesh.py:107-111)
    return f


def half_width_voxels(voxel_size, half_width=None):
    """the narrow band in voxels (reference sdf/mesh.py:73-77): 3, or ceil(half_width / voxel_size) if that is larger"""
    hw = 3
    if half_width is not None:
        hw = max(hw, int(np.ceil(half_width / voxel_size)))
    return hw


def level_set(points, triangles, voxel_size, half_width=None):
    """`Mesh.sdf` with the voxelisation on the device (csrc/sdf_level_set.hip) instead of OpenVDB's: the grid_sdf of the
    dense narrow-band grid of the mesh, cropped to the voxels with |value| < background like the reference's
    `evalActiveVoxelBoundingBox` + `copyToArray` (reference sdf/mesh.py:79-92).  The returned SDF3 carries the grid:
    `f.array`, `f.xyz`, `f.ijk0` (index of array[0, 0, 0]) and `f.background`."""
    from . import engine
    points = np.asarray(points, dtype=np.float64)
    hw = half_width_voxels(voxel_size, half_width)
    ijk0, A = engine.get_engine().mesh_level_set(points, triangles, voxel_size, hw)
    size = np.array(A.shape)
    ijk1 = ijk0 + size - 1
    p0, p1 = ijk0 * float(voxel_size), ijk1 * float(voxel_size)     # indexToWorld of a linear transform
    xyz = tuple(np.linspace(p0[i], p1[i], size[i]) for i in range(3))
    background = float(np.float32(hw * voxel_size))
    lo, hi = points.min(axis=0), points.max(axis=0)
    f = grid_sdf(xyz, A, background, (tuple(lo.tolist()), tuple(hi.tolist())))
    f.ijk0, f.background = ijk0, background
    return f


class Mesh:
    """reference sdf/mesh.py:8-62: points (V, 3), triangles (T, 3) and rigid / scaling transforms"""

    def __init__(self, points, triangles):
        self.points = points
        self.triangles = triangles

    @classmethod
    def from_file(cls, path):
        import meshio
        m = meshio.read(path)
        return cls(m.points, m.cells[0].data)

    @classmethod
    def from_stl(cls, path):
        """a binary STL (80-byte header, u32 count, 50-byte records) without meshio, its vertices welded like the
        reference's `_mesh` welds a soup (reference sdf/core.py:160-164): np.unique(points, axis=0, return_inverse=True)"""
        with open(path, 'rb') as fp:
            data = fp.read()
        if len(data) < 84:
            raise ValueError('%s: %d bytes is too short for a binary STL' % (path, len(data)))
        n = int(np.frombuffer(data, dtype='<u4', count=1, offset=80)[0])
        if len(data) != 84 + 50 * n:
            raise ValueError('%s: %d bytes, but a binary STL of %d triangles has %d' % (path, len(data), n, 84 + 50 * n))
        rec = np.frombuffer(data, dtype=np.dtype([('normal', '<f4', 3), ('points', '<f4', (3, 3)), ('attr', '<u2')]), count=n, offset=84)
        points, cells = np.unique(rec['points'].reshape(-1, 3).astype(np.float64), axis=0, return_inverse=True)
        return cls(points, np.asarray(cells).reshape((-1, 3)))

    def measure(self, origin=None):
        """volume, area, centroid, inertia and the edge census of this mesh, taken on the device (sdf_amd/measure.py)"""
        from .measure import measure_soup
        return measure_soup(np.asarray(self.points, dtype=np.float64)[np.asarray(self.triangles)], origin)

    def thickness(self, f, step=None, start=None, min_step=None, t_far=None, max_steps=256, refine=16, normal_eps=None, step_scale=1.0):
        """the walls of this mesh measured in the field `f` (sdf_amd/thickness.py): a `Thickness` over the
        vertices of the soup welded on the device.  A file has no sampling grid, so `step` must be given (start = min_step = a
        quarter of it), or start and min_step themselves; t_far defaults to the diagonal of this mesh's bounding box and normal_eps
        to 1e-4 x half of it."""
        from .thickness import default_params, thickness_of_soup
        pts = np.asarray(self.points, dtype=np.float64)
        if len(pts) == 0:
            raise ValueError('thickness: the mesh has no vertices')
        steps3 = None if step is None else tuple(np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)).tolist())
        params = default_params((pts.min(axis=0), pts.max(axis=0)), steps3, start, min_step, t_far, normal_eps)
        return thickness_of_soup(pts[np.asarray(self.triangles)], f, step_scale=step_scale, max_steps=max_steps, refine=refine, **params)

    def curvature(self, f, step=None, eps=None):
        """the curvature of the field `f` at the vertices of this mesh (sdf_amd/curvature.py): a `Curvature`
        over the vertices of the soup welded on the device.  A file has no sampling grid, so `step` must be given (eps = the
        smallest of its components: curvature at the scale the mesh can show), or eps itself."""
        from .curvature import curvature_of_soup, default_eps
        pts = np.asarray(self.points, dtype=np.float64)
        if len(pts) == 0:
            raise ValueError('curvature: the mesh has no vertices')
        steps3 = None if step is None else tuple(np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)).tolist())
        return curvature_of_soup(pts[np.asarray(self.triangles)], f, default_eps(steps3, eps))

    def deviation(self, f, order=2):
        """how far this mesh lies from the zero set of the field `f`, sampled on the device on every triangle (sdf_amd/deviation.py,
        DESIGN.md section 4q): a `Deviation`"""
        from .deviation import deviation_of_soup
        return deviation_of_soup(np.asarray(self.points, dtype=np.float64)[np.asarray(self.triangles)], f, order)

    def snap(self, f, step=None, eps=None, tol=None, max_move=None, iters=4):
        """a new Mesh: this one with its vertices put back on the zero set of the field `f` on the device (sdf_amd/deviation.py,
        DESIGN.md section 4q); it carries `snap_status`, `snap_residual` (per welded vertex) and `snap_stats`.  A file has no sampling
        grid, so `step` must be given (tol = 1e-3 x the smallest step, max_move = the diagonal of one cell), or tol and max_move
        themselves; eps defaults to 1e-4 x the half-diagonal of this mesh's bounding box"""
        from .deviation import snap_of_soup, snap_params
        pts = np.asarray(self.points, dtype=np.float64)
        if len(pts) == 0:
            raise ValueError('snap: the mesh has no vertices')
        if step is None and (tol is None or max_move is None):
            raise ValueError('snap: give step, or tol and max_move')
        steps3 = (1.0, 1.0, 1.0) if step is None else tuple(np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)).tolist())
        over = {k: v for k, v in (('eps', eps), ('tol', tol), ('max_move', max_move), ('iters', iters)) if v is not None}
        par = snap_params(over, (pts.min(axis=0), pts.max(axis=0)), steps3)
        q, cells, status, residual, stats = snap_of_soup(pts[np.asarray(self.triangles)], f, **par)
        out = Mesh(q, cells)
        out.snap_status, out.snap_residual, out.snap_stats = status, residual, stats
        return out

    def overhangs(self, directions=(0.0, 0.0, 1.0), angle=45.0, bed_tolerance=None, classes=False):
        """build directions rated for this mesh on the device (sdf_amd/overhang.py): an `Overhangs`.
        directions: one vector, an array (K, 3) or an int n for the six axes and n spiral points; a file has no sampling grid, so
        bed_tolerance=None is 0.0"""
        from .overhang import overhangs_soup
        return overhangs_soup(np.asarray(self.points, dtype=np.float64)[np.asarray(self.triangles)], directions, angle, bed_tolerance, classes)

    def supports(self, f, directions=(0.0, 0.0, 1.0), step=None, angle=45.0, bed_tolerance=None, start=None, min_step=None, step_scale=1.0,
                 max_steps=256, refine=16, top=8):
        """the support rays of this mesh traced in the field `f` on the device (sdf_amd/supports.py): a
        `Supports`.  A file has no sampling grid, so `step` must be given (start = min_step = a quarter of it), or start and min_step
        themselves, and bed_tolerance=None is 0.0"""
        from .supports import supports_soup
        if step is not None:
            quarter = float(np.min(np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)))) / 4
            start = quarter if start is None else start
            min_step = quarter if min_step is None else min_step
        return supports_soup(np.asarray(self.points, dtype=np.float64)[np.asarray(self.triangles)], f, directions, angle,
                             0.0 if bed_tolerance is None else bed_tolerance, start, min_step, step_scale, max_steps, refine, top)

    def shells(self):
        """the connected shells of this mesh (sdf_amd/shells.py `Shells`), labelled on the device.  The soup is welded there again:
        `vertex_shell` is over THAT weld's vertices (lexicographic order), `triangle_shell` over this mesh's triangles"""
        from .shells import shells_of_soup
        return shells_of_soup(np.asarray(self.points, dtype=np.float64)[np.asarray(self.triangles)])

    def simplify(self, cell, origin=None, reg=1e-3):
        """this mesh simplified on the device (sdf_amd/simplify.py): a new Mesh of the welded result.  cell: the
        edge of a cluster, a scalar or one per axis; origin: the corner of the clustering grid (default: the minimum of the bounding
        box); reg: the regularisation of the quadric towards the mean of a cluster's vertices"""
        from . import core
        pts = np.asarray(self.points, dtype=np.float64)
        c = np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,)).copy()
        o = pts.min(axis=0) if origin is None and len(pts) else np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
        with core.adopted(pts[np.asarray(self.triangles)]) as mesh:
            small = mesh.simplify(o, c, reg)
            try:
                points, cells = small.weld()
                return Mesh(np.array(points), np.array(cells))
            finally:
                small.close()

    def simplify_adaptive(self, cell, tolerance, levels=5, origin=None, reg=1e-3):
        """this mesh simplified to a tolerance on the device (sdf_amd/simplify.py): a new Mesh of the welded
        result.  cell: the edge of the FINEST cluster, a scalar or one per axis; tolerance: how far, in this mesh's units, a
        cluster's vertex may lie from the planes of the triangles it replaces (a squared-area-weighted root mean square, not a
        Hausdorff bound); levels: the clusters double in edge that many times, 0 .. 10; origin: the corner of the clustering grids
        (default: the minimum of the bounding box); reg: as for `simplify`"""
        from . import core
        pts = np.asarray(self.points, dtype=np.float64)
        c = np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,)).copy()
        o = pts.min(axis=0) if origin is None and len(pts) else np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
        with core.adopted(pts[np.asarray(self.triangles)]) as mesh:
            small = mesh.simplify_adaptive(o, c, tolerance, levels, reg)
            try:
                points, cells = small.weld()
                return Mesh(np.array(points), np.array(cells))
            finally:
                small.close()

    def mend(self):
        """this mesh mended on the device (sdf_amd/mend.py): a new Mesh of the welded result, without
        duplicate triangles and without the oppositely wound pairs that `simplify` leaves where a wall is thinner than a cluster"""
        from . import core
        pts = np.asarray(self.points, dtype=np.float64)
        with core.adopted(pts[np.asarray(self.triangles)]) as mesh:
            mended = mesh.mend()
            try:
                points, cells = mended.weld()
                return Mesh(np.array(points), np.array(cells))
            finally:
                mended.close()

    @property
    def bounding_box(self):
        lo, hi = self.points.min(axis=0), self.points.max(axis=0)
        return (tuple(lo.tolist()), tuple(hi.tolist()))

    @property
    def size(self):
        lo, hi = self.points.min(axis=0), self.points.max(axis=0)
        return tuple((hi - lo).tolist())

    def transformed(self, matrix):
        h = np.hstack([self.points, np.ones((self.points.shape[0], 1))])
        return Mesh((h @ np.array(matrix).T)[:, :3], self.triangles)

    def scaled(self, scale):
        try:
            sx, sy, sz = scale
        except TypeError:
            sx = sy = sz = scale
        return self.transformed([[sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, sz, 0], [0, 0, 0, 1]])

    def translated(self, offset):
        dx, dy, dz = offset
        return self.transformed([[1, 0, 0, dx], [0, 1, 0, dy], [0, 0, 1, dz], [0, 0, 0, 1]])

    def positioned(self, position, anchor):
        lo, hi = map(np.array, self.bounding_box)
        return self.translated(position - (lo + (hi - lo) * anchor))

    def centered(self):
        return self.positioned((0, 0, 0), (0.5, 0.5, 0.5))

    def sdf(self, voxel_size, half_width=None, voxelizer='openvdb'):
        """reference sdf/mesh.py:64-113; the voxelisation is OpenVDB's (host, like the reference) unless
        voxelizer='device' (`level_set`: on the device, no OpenVDB); the per-sample lookup runs on the device"""
        if voxelizer == 'device':
            return level_set(self.points, self.triangles, voxel_size, half_width)
        if voxelizer != 'openvdb':
            raise ValueError("voxelizer must be 'openvdb' or 'device', got %r" % (voxelizer,))
        import pyopenvdb as vdb

        grid = vdb.FloatGrid.createLevelSetFromPolygons(
            self.points, triangles=self.triangles,
            transform=vdb.createLinearTransform(voxelSize=voxel_size), halfWidth=half_width_voxels(voxel_size, half_width))
        v0, v1 = grid.evalActiveVoxelBoundingBox()
        ijk0, ijk1 = np.array(v0, dtype=int), np.array(v1, dtype=int)
        size = ijk1 - ijk0 + 1
        p0, p1 = grid.transform.indexToWorld(ijk0), grid.transform.indexToWorld(ijk1)
        xyz = tuple(np.linspace(p0[i], p1[i], size[i]) for i in range(3))
        A = np.zeros(size, dtype=np.float32)
        grid.copyToArray(A, ijk=ijk0)
        f = grid_sdf(xyz, A, grid.background, self.bounding_box)
        f.grid = grid
        return f
