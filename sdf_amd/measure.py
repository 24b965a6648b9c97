"""A mesh measured on the device (not in the reference): `measure(f)` meshes a model, keeps the soup on the
GPU and returns its volume, surface area, centre of mass, inertia tensor and bounds -- from the raw totals of `Mesh.moments`
(sdf_mesh_moments: one pass over the soup, a fixed summation tree) -- and the edge census of the welded mesh (`Mesh.edge_census`,
sdf_mesh_edge_census): is it closed, consistently oriented, free of non-manifold edges, and what is its Euler characteristic.
tests/measure_ref.py is the definition; `derive` restates its few lines of host arithmetic."""
import collections

import numpy as np

from .meshfile import frozen as _frozen

Measurement = collections.namedtuple('Measurement', (
    'volume', 'area', 'centroid', 'inertia', 'bounds', 'triangles', 'zero_area_triangles', 'nonfinite_triangles',
    'vertices', 'faces', 'collapsed', 'edges', 'paired', 'boundary', 'misoriented', 'nonmanifold', 'euler', 'closed', 'oriented',
    'origin', 'sums'))
Measurement.__doc__ = """what `measure` returns (immutable).  volume, area: float; centroid (3,), inertia (3, 3) at unit density about
the centroid (NaN when the volume is not positive or a triangle is not finite); bounds ((x0, y0, z0), (x1, y1, z1)) of the soup;
triangles, zero_area_triangles, nonfinite_triangles; the census: vertices, faces, collapsed, edges = paired + boundary +
misoriented + nonmanifold, euler = vertices - edges + faces, closed = no boundary and no non-manifold edge, oriented = no
misoriented edge; origin (3,) and sums (11,): the reference point and the raw totals the values come from."""


def derive(m):
    """area, volume, centroid, inertia from the totals of `Mesh.moments`: the factors 1/2, 1/6, 1/24, 1/120 meet the totals here,
    once, in the order of tests/measure_ref.py::derive"""
    s = np.asarray(m['sums'], dtype=np.float64)
    o = np.asarray(m['origin'], dtype=np.float64)
    area = s[0] / 2.0
    volume = s[1] / 6.0
    if not (volume > 0) or m['nonfinite'] > 0:
        return {'area': area, 'volume': volume, 'centroid': np.full(3, np.nan), 'inertia': np.full((3, 3), np.nan)}
    with np.errstate(all='ignore'):
        d = s[2:5] / (4.0 * s[1])
        centroid = d + o
        q = s[5:11] / 120.0
        xx, yy, zz = q[0] - volume * d[0] * d[0], q[1] - volume * d[1] * d[1], q[2] - volume * d[2] * d[2]
        xy, xz, yz = q[3] - volume * d[0] * d[1], q[4] - volume * d[0] * d[2], q[5] - volume * d[1] * d[2]
        inertia = np.array([[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]])
    return {'area': area, 'volume': volume, 'centroid': centroid, 'inertia': inertia}


def measure_mesh(mesh, origin=None):
    """the Measurement of a device mesh (`engine.Mesh`): moments, derived values, census (welds if needed)"""
    m = mesh.moments(origin)
    c = mesh.edge_census()
    d = derive(m)
    lo, hi = m['box']
    return Measurement(
        volume=float(d['volume']), area=float(d['area']), centroid=_frozen(d['centroid'], np.float64), inertia=_frozen(d['inertia'], np.float64),
        bounds=(tuple(lo.tolist()), tuple(hi.tolist())), triangles=m['triangles'], zero_area_triangles=m['zero_area'],
        nonfinite_triangles=m['nonfinite'], origin=_frozen(m['origin'], np.float64), sums=_frozen(m['sums'], np.float64), **c)


def measure(sdf, origin=None, keep=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, snap=False, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and measure the
    mesh there: nothing but the result crosses the link.  origin: the point the moments are taken about (default: the midpoint of
    the soup's bounding box, which keeps the cancellation small for a model far from the world's origin; the results are given
    about the centroid either way).  keep: measure only these connected shells of the mesh (`shells.resolve_keep`; `measure_shells`
    gives every shell its own Measurement).  simplify: measure the mesh simplified in clusters of simplify^3 grid cells, after keep
    (`sdf_amd/simplify.py`; duplicate or oppositely wound triangles that the clustering made show up in the census unless `mend`).
    simplify_tolerance, simplify_levels: measure the mesh simplified to that tolerance instead (model units).
    mend: True -- measure the mesh mended after keep and simplify (`sdf_amd/mend.py`).  snap: True or a dict -- measure the mesh whose
    vertices were put back on the zero set after simplify (`sdf_amd/deviation.py`).  A multi-process run whose gathered soup is on the host raises NotImplementedError."""
    from . import core
    with core.meshed(sdf, keep=keep, **core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap)) as m:
        core.need_device_mesh(m.mesh, 'measure', 'the measurements are made')
        return measure_mesh(m.mesh, origin)


def measure_soup(soup, origin=None):
    """the Measurement of a float64 soup (T, 3, 3) on the host: uploaded (torch), adopted and measured on the device"""
    from . import core
    with core.adopted(soup) as mesh:
        return measure_mesh(mesh, origin)
