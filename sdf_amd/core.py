"""Sampling + meshing driver: the drop-in for reference sdf/core.py.

Same entry points and keyword arguments as the reference (``generate`` sdf/core.py:84-150,
``save`` :152-158, ``sample_slice`` :202-232, ``show_slice`` :234-244), but the batch
loop, the sparse skip test, SDF sampling and marching cubes all run in HIP kernels behind
the C ABI of include/sdf_hip.h (see sdf_amd/engine.py).  What stays on the host is what
the reference also does once per call in scalar Python: bounds -> step -> ``np.arange``
axes (kept in NumPy float64 so the grid is bit-identical to the reference's).

Differences a caller can observe:
* ``generate`` returns ONE float64 ndarray of shape (3*T, 3) instead of a Python list of
  3*T tiny arrays (same ``len``, indexing, ``write_binary_stl`` and ``np.unique``
  behaviour).
* ``workers`` does not drive the sampling (the device runs every batch concurrently); it is the
  number of host threads that turn the device's 16-byte triangle records into the float64 rows
  of the returned array (``sdf_mesh_emit_host_workers``; at most 32 -- more were measured to be no faster).
* when ``torch.distributed`` is initialised with world_size > 1 the surviving batches are
  sharded over the ranks and the triangle buffers all-gathered (sdf_amd/dist.py), so
  every rank still returns the complete soup in reference order.
"""
import collections
import contextlib
import multiprocessing
import os
import time

import numpy as np

from . import stl

WORKERS = multiprocessing.cpu_count()
SAMPLES = 2 ** 22
BATCH_SIZE = 32


def _marching_cubes(volume, level=0):
    """skimage's Lewiner marching cubes of a host volume, as the triangle soup (3T, 3) float32 in index
    coordinates (reference sdf/core.py:16-18: `verts[faces].reshape((-1, 3))`), on the device
    (`sdf_marching_cubes_host`: k_mc_rows / k_scan_rows / k_mc_emit).  Raises what skimage raises: ValueError
    for a volume that is not 3-D, smaller than 2 x 2 x 2 or whose range does not contain `level`, RuntimeError
    when no surface is found -- `_worker` turns any of them into an empty batch, like the reference's.
    The reference only ever passes level 0; another level is subtracted in float64 on the float32-cast
    volume (skimage's own order) and the result cast back to float32 for the device."""
    from . import engine
    vol = np.asarray(volume)
    if vol.ndim != 3:
        raise ValueError('Input volume should be a 3D numpy array.')
    if min(vol.shape) < 2:
        raise ValueError('Input array must be at least 2x2x2.')
    level = float(level)
    if level < vol.min() or level > vol.max():
        raise ValueError('Surface level must be within volume data range.')
    v32 = vol.astype(np.float32)
    if level != 0.0:
        v32 = (v32.astype(np.float64) - level).astype(np.float32)
    soup = engine.get_engine().marching_cubes(v32)
    if len(soup) == 0:
        raise RuntimeError('No surface found at the given iso value.')
    return soup


def _skip(sdf, job):
    """the sparse skip test of one batch (reference sdf/core.py:28-43): True when the batch cannot hold
    surface.  The nine probes -- centre and the 8 corners of the batch's box -- are evaluated in one call of
    `sdf` (on the device for the library's own nodes); the comparisons are the reference's.  `generate` itself
    runs the same test for every batch of a grid in one launch (`k_skip`)."""
    X, Y, Z = job
    lo = np.array([X[0], Y[0], Z[0]])
    hi = np.array([X[-1], Y[-1], Z[-1]])
    mid = (lo + hi) / 2
    sel = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=bool)   # itertools.product order
    probes = np.vstack([mid[None, :], np.where(sel, hi, lo)])
    values = np.asarray(sdf(probes)).reshape(-1)
    if abs(values[0]) <= np.linalg.norm(mid - lo):
        return False
    corners = values[1:]
    return bool(np.all(corners > 0) if corners[0] > 0 else np.all(corners < 0))


def _worker(sdf, job, step, sparse):
    """one batch of `generate` (reference sdf/core.py:45-60): None when the skip test drops it, [] when it
    has no surface, else its triangles `points * scale + offset` as a (3T, 3) float64 array.  The job is meshed
    as a grid of its own whose first batch is the job (batch_size = its longest axis - 1; what lies behind it
    are slivers one sample thick, which have no cells): the same fused kernels `generate` uses."""
    from . import engine
    X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in job)
    if min(len(X), len(Y), len(Z)) < 2:
        return None if (sparse and len(X) and len(Y) and len(Z) and _skip(sdf, job)) else []
    bs = max(len(X), len(Y), len(Z)) - 1
    mesh = engine.get_engine().generate(sdf, X, Y, Z, bs, sparse)
    try:
        if sparse and mesh.kinds()[0] == 0:
            return None
        points = mesh.points()
    finally:
        mesh.close()
    return points if len(points) else []


def _cartesian_product(*arrays):
    """(N, d) points, first axis slowest (reference sdf/core.py:20-26); host helper kept
    for API compatibility -- the device generates grid points from the axes itself"""
    grids = np.meshgrid(*arrays, indexing='ij')
    return np.stack([g.reshape(-1) for g in grids], axis=-1)


def _estimate_bounds(sdf):
    """iterative 16^3 shrink from +-1e9 (reference sdf/core.py:62-82), on the device"""
    from . import engine
    eng = engine.get_engine()
    tape = eng.tape_for(sdf)
    if eng.precision == engine.PRECISION_F64:        # the whole loop in one launch (k_estimate_bounds)
        b = eng.estimate_bounds(tape)
        if b is not None:
            return b
    # (float32 sampling, and models with user closures: the reference's loop, the probes evaluated by eval_grid)
    s = 16
    x0 = y0 = z0 = -1e9
    x1 = y1 = z1 = 1e9
    prev = None
    for i in range(32):
        X = np.linspace(x0, x1, s)
        Y = np.linspace(y0, y1, s)
        Z = np.linspace(z0, z1, s)
        d = np.array([X[1] - X[0], Y[1] - Y[0], Z[1] - Z[0]])
        threshold = np.linalg.norm(d) / 2
        if threshold == prev:
            break
        prev = threshold
        volume = eng.eval_grid(tape, X, Y, Z)
        reach = np.abs(volume)
        if eng.precision != engine.PRECISION_F64:
            # float32 values: 16 units of 2^-24 max(|v|, |p|inf, 1) are taken off before the comparison, as k_estimate_bounds_w<float>
            # does (csrc/sdf_bounds.hip says why: without it no probe of the first round is within the threshold)
            far = np.maximum(np.maximum(np.abs(X)[:, None, None], np.abs(Y)[None, :, None]), np.abs(Z)[None, None, :])
            reach = reach - 2.0 ** -20 * np.maximum(np.maximum(reach, far), 1.0)
        where = np.argwhere(reach <= threshold)
        x1, y1, z1 = (x0, y0, z0) + where.max(axis=0) * d + d / 2
        x0, y0, z0 = (x0, y0, z0) + where.min(axis=0) * d - d / 2
    return ((x0, y0, z0), (x1, y1, z1))


def grid_axes(bounds, step=None, samples=SAMPLES):
    """bounds/step/samples -> (X, Y, Z, (dx, dy, dz)) exactly as reference sdf/core.py:94-112"""
    (x0, y0, z0), (x1, y1, z1) = bounds
    if step is None and samples is not None:
        volume = (x1 - x0) * (y1 - y0) * (z1 - z0)
        step = (volume / samples) ** (1 / 3)
    try:
        dx, dy, dz = step
    except TypeError:
        dx = dy = dz = step
    X = np.arange(x0, x1, dx)
    Y = np.arange(y0, y1, dy)
    Z = np.arange(z0, z1, dz)
    return X, Y, Z, (dx, dy, dz)


def need_device_mesh(mesh, name, words):
    """the refusal, in `name`'s words, of a soup that a multi-process run gathered on the host: there is no mesh on the device to read"""
    if mesh is None:
        raise NotImplementedError('%s: the soup of this multi-process run was gathered on the host; %s on the device only '
                                  '(run it in one process, or with a device-resident exchange)' % (name, words))


Meshed = collections.namedtuple('Meshed', ('mesh', 'points', 'tape', 'engine', 'bounds', 'stats', 'simplify_stats'), defaults=(None,))
Meshed.__doc__ = """what `meshed` yields.  mesh: the `engine.Mesh` on the device (the selection under keep=, the simplified mesh under
simplify=, the mended mesh under mend=True -- its statistics ride on it: `mesh.mend_stats`), or None when a multi-process run gathered its soup on the host -- then points is that soup, (3T, 3) float64; tape,
engine, bounds, stats: the call's; simplify_stats: the dict of `engine.Mesh.simplify` -- of `engine.Mesh.simplify_adaptive` under
simplify_tolerance= --, or None without either.  Under snap= the statistics of `engine.Mesh.snap` ride on the mesh, like mend's:
`mesh.snap_stats` (through a mend as well)."""


@contextlib.contextmanager
def meshed(
        sdf,
        step=None, bounds=None, samples=SAMPLES,
        workers=WORKERS, batch_size=BATCH_SIZE,
        verbose=True, sparse=True, *, keep=None, simplify=None, mend=False, to_host=False, simplify_tolerance=None, simplify_levels=5, snap=False,
        dual=False):
    """the one path from a model to its mesh on the device: the arguments of `generate`, `keep` (only these
    connected shells, `shells.resolve_keep`: the device mesh is labelled, the kept shells are compacted into a mesh of their own
    and THAT is yielded; section 4h), `simplify` (a real number k > 0, `simplify.check_simplify`: after keep, the mesh is simplified on
    the device in clusters of k^3 grid cells, `engine.Mesh.simplify`, and the simplified mesh is what is yielded and what the closing
    line counts; section 4j), `simplify_tolerance` and `simplify_levels` (a real number >= 0 in model units and an integer 0 .. 10,
    `simplify.check_adaptive`: in the place of the uniform clustering the mesh is simplified to that tolerance on the levels of
    simplify x 2^L grid cells, L = 0 .. simplify_levels, `engine.Mesh.simplify_adaptive`; simplify is then the finest cluster and
    defaults to 1; section 4p), `snap` (False, True or a dict of eps, tol, max_move, iters, `deviation.check_snap_option`: after
    simplify and before mend, the welded vertices are put back on the zero set of the field by Newton steps on the device,
    `engine.Mesh.snap`, and the moved mesh is what is yielded -- two vertices that land on one point make a collapsed triangle, which
    mend drops; eps defaults to the preview's normal_eps, tol to 1e-3 x the smallest grid step, max_move to the diagonal of one
    cluster cell, of one grid cell without simplify, iters to 4; section 4q), `mend` (False or True, `mend.check_mend`: after keep and after simplify -- simplifying is what makes the
    pairs -- duplicate triangles are dropped and oppositely wound pairs cancel on the device, `engine.Mesh.mend`, and the mended mesh
    is what is yielded and what the closing line counts; section 4k), `dual` (False, True or a dict of eps and reg,
    `dual.check_dual_option`: the mesh is made by dual contouring of the field in the place of marching cubes, on the same grid,
    `engine.Engine.generate_dual` -- one vertex per grid cell that the surface crosses, placed by the quadric of the field's tangent
    planes, so creases stay sharp; eps, the step of the normals, defaults to the preview's normal_eps, reg to 1e-3; the grid is
    sampled densely: batch_size, sparse and workers do not steer it (batch_size only sizes the blocks that the closing line counts
    as nonempty / empty); every stage above works on the result unchanged, and `generate.last_dual` holds its eight counters; one
    process only; section 4u) and `to_host` (the caller wants the float64 soup on the host: the triangles then travel as
    16-byte records).  Yields a `Meshed`, which the readers below take; closes what it opened on the way out, and after a body
    that did not raise prints the two closing lines of the reference and sets `generate.last_stats`."""
    from . import engine, dist
    if keep is not None:
        from .shells import check_keep, resolve_keep, shells_of_mesh
        check_keep(keep)      # (before anything is meshed)
    from .simplify import check_adaptive, resolve_cell
    simplify, simplify_tolerance, simplify_levels = check_adaptive(simplify, simplify_tolerance, simplify_levels)      # (before anything is meshed)
    from .mend import check_mend
    mend = check_mend(mend)      # (before the engine is asked for)
    from .deviation import check_snap_option, snap_params
    snap = check_snap_option(snap)      # (None: the call without it)
    from .dual import check_dual_option, dual_params
    dual = check_dual_option(dual)      # (None: the call without it)
    start = time.time()
    eng = engine.get_engine()
    tape = eng.tape_for(sdf)

    if bounds is None:
        bounds = _estimate_bounds(tape)      # (the tape lowered above: lowering the model a second time is 0.08 ms of a 2.5 ms call)
    (x0, y0, z0), (x1, y1, z1) = bounds
    X, Y, Z, (dx, dy, dz) = grid_axes(bounds, step, samples)

    if verbose:
        print('min %g, %g, %g' % (x0, y0, z0))
        print('max %g, %g, %g' % (x1, y1, z1))
        print('step %g, %g, %g' % (dx, dy, dz))

    s = batch_size
    num_batches = (-(-len(X) // s)) * (-(-len(Y) // s)) * (-(-len(Z) // s))
    if verbose:
        def overlapped(n):       # samples counted with the 1-sample batch overlap (core.py:121-122)
            return sum(min(s + 1, n - i) for i in range(0, n, s))
        num_samples = overlapped(len(X)) * overlapped(len(Y)) * overlapped(len(Z))
        print('%d samples in %d batches with %d workers' % (num_samples, num_batches, workers))

    mesh = points = soup = simplify_stats = None
    try:
        if dual is not None:
            if dist.world_size() > 1:
                need_device_mesh(None, 'dual', 'a field is dual-contoured')
            mesh = eng.generate_dual(tape, X, Y, Z, *dual_params(dual, bounds), batch_size=batch_size)
            stats = mesh.stats()
            generate.last_dual = mesh.dual_stats
        elif dist.world_size() > 1:
            soup, stats = dist.generate_sharded_device(eng, tape, X, Y, Z, batch_size, sparse)
            if not to_host and getattr(soup, 'is_cuda', False):
                # the gathered soup stays on the device (and alive, as `soup`, while the mesh over it is read)
                import torch
                torch.cuda.current_stream(soup.device).synchronize()
                mesh = eng.adopt_soup(soup.data_ptr(), soup.numel() // 9)
            else:
                points = soup.cpu().numpy().reshape(-1, 3)
        else:
            mesh = eng.generate(tape, X, Y, Z, batch_size, sparse, records=to_host)
            stats = mesh.stats()

        # the stages, each from the current mesh to the new one; the frame below them refuses, calls, closes and hands over
        def kept(mesh):
            # (choosing by size brings the per-shell counts over the link and nothing else; a callable is handed the whole `Shells`)
            got = shells_of_mesh(mesh) if callable(keep) else mesh.shell_summary()['triangles']
            return mesh.select(resolve_keep(keep, got))

        def simplified(mesh):
            nonlocal simplify_stats
            origin, cell = resolve_cell(simplify, X, Y, Z, (dx, dy, dz))
            small = mesh.simplify(origin, cell) if simplify_tolerance is None else mesh.simplify_adaptive(origin, cell, simplify_tolerance, simplify_levels)
            simplify_stats = small.simplify_stats
            return small

        def snapped(mesh):
            return mesh.snap(tape, **snap_params(snap, bounds, (dx, dy, dz), simplify))

        def mended(mesh):
            new = mesh.mend()
            if snap is not None:
                new.snap_stats = mesh.snap_stats
            return new

        for name, asked, words, stage in (('keep', keep is not None, 'shells are found and selected', kept),
                                          ('simplify', simplify is not None, 'a mesh is simplified', simplified),
                                          ('snap', snap is not None, 'a mesh is snapped', snapped),
                                          ('mend', mend, 'a mesh is mended', mended)):
            if asked:
                need_device_mesh(mesh, name, words)
                new = stage(mesh)
                mesh.close()
                mesh = new
        yield Meshed(mesh, points, tape, eng, bounds, stats, simplify_stats)
        triangles = mesh.n_triangles if mesh is not None else len(points) // 3
    finally:
        if mesh is not None:
            mesh.close()

    if verbose:
        print('%d skipped, %d empty, %d nonempty' % (stats['skipped'], stats['empty'], stats['nonempty']))
        seconds = time.time() - start
        print('%d triangles in %g seconds' % (triangles, seconds))
    generate.last_stats = stats


def pipeline_kwargs(generate_kwargs, simplify=None, simplify_tolerance=None, simplify_levels=5, mend=False, snap=False, dual=False):
    """the keywords of `meshed` for a facade's call: its generate_kwargs and, of the pipeline's options, those that are not the
    default.  A default is left out, not passed: `meshed` is looked up at call time, and what stands in for it -- the stand-ins of
    the host tests, a caller's own wrapper -- then sees the call that was made and needs no knowledge of a keyword it was never
    given; only the defaults themselves are left out, what merely compares equal (5.0, True, None for False) goes on for
    `meshed` to judge.  `overhangs` and `supports` have no snap= and pass none: one in their generate_kwargs rides on as it is."""
    kw = dict(generate_kwargs)
    if simplify is not None:
        kw['simplify'] = simplify
    if not (simplify_tolerance is None and isinstance(simplify_levels, int) and not isinstance(simplify_levels, bool) and simplify_levels == 5):
        kw.update(simplify_tolerance=simplify_tolerance, simplify_levels=simplify_levels)
    if mend is not False:
        kw['mend'] = mend
    if snap is not False:
        kw['snap'] = snap
    if dual is not False:
        kw['dual'] = dual
    return kw


def grid_steps(m, call):
    """(dx, dy, dz) of the meshing call that the `Meshed` m came from: out of its bounds and the `step` and `samples` among the
    call's keywords, as `meshed` computed them"""
    return grid_axes(m.bounds, call.get('step'), call.get('samples', SAMPLES))[3]


def default_normal_eps(bounds):
    """the step of the central difference that gives a normal, 1e-4 x the half-diagonal of the bounds: the preview's value
    (render.render_buffers), so that a file, a probe and a preview of one model see the same normals"""
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    return 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)


@contextlib.contextmanager
def adopted(soup):
    """a float64 soup (T, 3, 3) on the host as an `engine.Mesh`: uploaded (torch) and adopted for the life of the context"""
    import torch
    from . import engine
    eng = engine.get_engine()
    host = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 9)
    buf = torch.from_numpy(host).to('cuda:%d' % eng.device) if len(host) else None
    torch.cuda.synchronize()
    mesh = eng.adopt_soup(buf.data_ptr() if len(host) else 0, len(host))
    try:
        yield mesh
    finally:
        mesh.close()


# -- the readers of a `Meshed`: each one names what it does with a soup that a multi-process run gathered on the host --

def read_soup(m, workers=0):
    """(3T, 3) float64 on the host: the 16-byte records come over and `workers` host threads make the float64 rows from them --
    the one place the reference's `workers=` still means something here"""
    return m.mesh.points(min(int(workers), 32) if workers else 0) if m.mesh is not None else m.points


def read_stl_records(m):
    """T x 50 bytes, made on the device (k_stl); byte-identical to `stl.stl_records` of the soup -- tests/test_gpu.py"""
    return m.mesh.stl_records() if m.mesh is not None else stl.stl_records(m.points).view(np.uint8).reshape(-1)


def read_weld(m):
    """(unique points, cells): sdf_mesh_weld, or the reference's np.unique over the 3T rows"""
    if m.mesh is not None:
        return m.mesh.weld()
    pts, cells = np.unique(m.points, axis=0, return_inverse=True)
    return pts, np.asarray(cells).reshape((-1, 3))


def read_export(m, normals=False, eps=None, ply=False):
    """what the indexed export takes: the weld, with `normals` the field's normals at the welded vertices (step eps, default 1e-4 x
    the half-diagonal of the bounds; k_vertex_normals) -- a dict of `n_vertices`, `n_faces`, `normals` ((U, 3) float64 or None),
    `n_flat` and, with `ply`, the device-packed PLY body `ply` = (vertex_bytes, face_bytes); otherwise `points`, `cells` of the weld.
    A soup gathered on the host takes its normals from the definition over eval_points and its PLY body from the host packer."""
    from . import engine, meshfile
    out = {'normals': None, 'n_flat': 0}
    if normals and eps is None:
        eps = default_normal_eps(m.bounds)
    mesh = m.mesh
    if mesh is None:
        pts, cells = read_weld(m)
        out.update(points=pts, cells=cells, n_vertices=len(pts), n_faces=len(cells))
        if normals:
            out['normals'], out['n_flat'] = meshfile.vertex_normals(engine.evaluator(m.engine, m.tape), pts, eps)
        if ply:
            out['ply'] = meshfile.ply_records(pts, cells, out['normals'])
        return out
    if normals:
        out['normals'], out['n_flat'] = mesh.vertex_normals(m.tape, eps)
    if ply:
        if normals and m.tape.tape.externs:      # (closures: their normals were taken on the host)
            out['points'], out['cells'] = mesh.weld()
            out['ply'] = meshfile.ply_records(out['points'], out['cells'], out['normals'])
        else:
            out['ply'] = mesh.ply_records(normals=bool(normals))
        out['n_vertices'], out['n_faces'] = len(out['ply'][0]) // (24 if normals else 12), mesh.n_triangles
    else:
        out['points'], out['cells'] = mesh.weld()
        out['n_vertices'], out['n_faces'] = len(out['points']), len(out['cells'])
    return out


def generate(
        sdf,
        step=None, bounds=None, samples=SAMPLES,
        workers=WORKERS, batch_size=BATCH_SIZE,
        verbose=True, sparse=True, *, dual=False):
    """reference sdf/core.py:84-150.  `batch_size` up to 512 (the reference takes any: a larger one is refused with a message; up
    to 32 runs the fused kernels, above that the batches go through device memory -- a model with user closures then hands its
    callback one whole tile at a time, (batch_size + 1)^3 points: 4.3 GB of pinned host memory at 512).  dual: True or a dict of
    eps and reg -- the soup of dual contouring in the place of marching cubes: sharp creases (`meshed`, DESIGN.md section 4u;
    not in the reference; `generate.last_dual` holds its counters)."""
    with meshed(sdf, step, bounds, samples, workers, batch_size, verbose, sparse, to_host=True, **({} if dual is False else {'dual': dual})) as m:
        return read_soup(m, workers)


generate.last_stats = None
generate.last_dual = None


def generate_mesh(sdf, normals=False, normal_eps=None, keep=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5,
                  snap=False, dual=False, **generate_kwargs):
    """the indexed mesh of `generate`: (points (U, 3) float64, cells (T, 3) int64, normals (U, 3) float64 or None) -- the soup
    welded on the device, as `save` welds it for every format but STL, and with normals=True the normalised central
    difference of the FIELD at every vertex (step normal_eps; default 1e-4 x the half-diagonal of the bounds, the preview's
    value).  The normals point outward for this library's winding; a vertex where the field has no gradient gets (0, 0, 0)
    (`generate_mesh.last_flat` counts them).  keep: only these connected shells of the mesh (`shells.resolve_keep`: 'largest', a
    count, a boolean mask over the shells, a callable).  simplify: a real number k > 0 -- the mesh simplified on the
    device in clusters of k^3 grid cells, after keep (`sdf_amd/simplify.py`; `generate_mesh.last_simplify` holds
    its statistics); the normals are then the field's at the NEW vertices.  mend: True -- after keep and simplify, duplicate triangles
    are dropped and oppositely wound pairs cancel (`sdf_amd/mend.py`; `generate_mesh.last_mend` holds the
    statistics of the last call that mended).  snap: True or a dict of eps, tol, max_move, iters -- after simplify and before mend the
    vertices are put back on the zero set of the field (`sdf_amd/deviation.py`; `generate_mesh.last_snap` holds
    the statistics of the last call that snapped); the normals are then the field's at the snapped vertices.  dual: True or a dict of
    eps and reg -- the mesh is made by dual contouring in the place of marching cubes, and every stage above works on it
    (`meshed`; `generate.last_dual` holds its counters).  Not in the reference."""
    with meshed(sdf, keep=keep, **pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap, dual)) as m:
        got = read_export(m, bool(normals), normal_eps)
        generate_mesh.last_simplify = m.simplify_stats
        if mend:
            generate_mesh.last_mend = m.mesh.mend_stats
        if getattr(m.mesh, 'snap_stats', None) is not None:
            generate_mesh.last_snap = m.mesh.snap_stats
    generate_mesh.last_flat = got['n_flat']
    return got['points'], got['cells'], got['normals']


generate_mesh.last_flat = 0
generate_mesh.last_simplify = None
generate_mesh.last_mend = None
generate_mesh.last_snap = None


def save(path, *args, normals=False, normal_eps=None, writer=None, keep=None, simplify=None, mend=False, thickness=False,
         simplify_tolerance=None, simplify_levels=5, snap=False, curvature=False, dual=False, **kwargs):
    """reference sdf/core.py:152-158.  `.ply` and `.obj` are also written without meshio (sdf_amd/meshfile.py), with
    normals=True carrying the field's normals at the vertices (step normal_eps, see `generate_mesh`); writer = 'native' /
    'meshio' picks one, None (default) is meshio where it imports and no normals are asked for, else native.  keep: write only
    these connected shells of the mesh -- 'largest', the n largest, a boolean mask over the shells, a callable (`shells.resolve_keep`;
    DESIGN.md section 4h) --, selected on the device before anything is written.  simplify: a real number k > 0 -- after keep, the mesh
    is simplified on the device in clusters of k^3 grid cells and the file holds the simplified mesh: about k^2 times fewer triangles
    cross the link and reach the disk (`sdf_amd/simplify.py`).  mend: True -- after keep and simplify, duplicate
    triangles are dropped and oppositely wound pairs cancel, and the file holds the mended mesh (`sdf_amd/mend.py`, DESIGN.md
    section 4k).  thickness: True, or a dict of the probe's arguments (start, min_step, t_far, step_scale, max_steps, refine) -- the
    vertices of a .ply file carry the wall thickness of the final mesh as `property float quality` (`sdf_amd/thickness.py`, DESIGN.md
    section 4l; the direction's step is normal_eps); the native writer only, any other extension or writer raises ValueError before
    anything is meshed, and the file's body is packed on the host: it is not the fast path.  May be combined with normals=True.
    snap: True or a dict of eps, tol, max_move, iters -- after simplify and before mend the vertices are put back on the zero set of
    the field, and the file holds the moved mesh (`sdf_amd/deviation.py`).  curvature: 'mean', 'gauss', 'k1',
    'k2' or 'max' (of k1 and k2 the one of larger magnitude, signed), or a dict of `quality` (one of these, default 'mean') and `eps`
    -- the vertices of a .ply file carry that curvature of the field at the final mesh's vertices as `property float quality`
    (`sdf_amd/curvature.py`; eps defaults to the smallest grid step), through the same door and under the same
    rules as thickness=; a file has one quality column, so thickness= and curvature= together raise ValueError.  dual: True or a dict
    of eps and reg -- the file holds the mesh of dual contouring in the place of marching cubes': sharp creases (`meshed`,
    DESIGN.md section 4u); every option above works on it."""
    from . import meshfile
    path = os.fspath(path)
    how = meshfile.choose_writer(path, writer, normals, bool(thickness), bool(curvature))
    ply = path.lower().endswith('.ply')
    call = dict(zip(('sdf', 'step', 'bounds', 'samples'), args), **kwargs)      # (the positional arguments of `meshed`, by name)
    if thickness:                 # (refused before anything is meshed, like the extension above)
        from .thickness import check_params, default_params, read_thickness
        probe = dict(thickness) if isinstance(thickness, dict) else {}
        unknown = set(probe) - {'start', 'min_step', 't_far', 'step_scale', 'max_steps', 'refine'}
        if unknown:
            raise ValueError('thickness: unknown probe arguments %s' % sorted(unknown))
        check_params(1.0 if normal_eps is None else normal_eps, probe.get('start', 1.0), probe.get('min_step', 1.0),
                     probe.get('t_far', np.finfo(np.float64).max), probe.get('step_scale', 1.0), probe.get('max_steps', 256), probe.get('refine', 16))
    if curvature:                 # (refused before anything is meshed, too)
        from .curvature import default_eps, quality_of, read_curvature, save_option
        which, curvature_eps = save_option(curvature)
    with meshed(*args, keep=keep, **pipeline_kwargs(kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap, dual)) as m:
        if curvature:
            got = read_export(m, bool(normals), normal_eps)
            quality = quality_of(read_curvature(m, default_eps(grid_steps(m, call), curvature_eps), with_mesh=False)[2], which)
        elif thickness:
            got = read_export(m, bool(normals), normal_eps)
            params = dict(default_params(m.bounds, grid_steps(m, call), probe.get('start'), probe.get('min_step'), probe.get('t_far'), normal_eps),
                          step_scale=float(probe.get('step_scale', 1.0)), max_steps=int(probe.get('max_steps', 256)), refine=int(probe.get('refine', 16)))
            quality = read_thickness(m, params, with_mesh=False)[2]
        elif how == 'native':
            got = read_export(m, bool(normals), normal_eps, ply)
        elif how == 'stl':
            records = read_stl_records(m)
        else:
            points, cells = read_weld(m)
    if thickness or curvature:
        vb, fb = meshfile.ply_records(got['points'], got['cells'], got['normals'], quality)
        meshfile.write_ply(path, vb, fb, got['n_vertices'], got['n_faces'], bool(normals), quality=True)
    elif how == 'native' and ply:
        meshfile.write_ply(path, got['ply'][0], got['ply'][1], got['n_vertices'], got['n_faces'], bool(normals))
    elif how == 'native':
        meshfile.write_obj(path, got['points'], got['cells'], got['normals'])
    elif how == 'stl':
        stl.write_stl_records(path, records)
    else:
        import meshio
        meshio.Mesh(points, [('triangle', cells)]).write(path)


def _mesh(points):
    """vertex weld of a host-side soup for non-STL formats (reference sdf/core.py:160-164; needs
    meshio).  `save` does not come through here: it welds on the device (`read_weld`)."""
    import meshio
    points, cells = np.unique(points, axis=0, return_inverse=True)
    cells = [('triangle', np.asarray(cells).reshape((-1, 3)))]
    return meshio.Mesh(points, cells)


def sample_slice(
        sdf, w=1024, h=1024,
        x=None, y=None, z=None, bounds=None):
    """a w x h image of the field on an axis-aligned plane (reference sdf/core.py:202-232)"""
    from . import engine
    eng = engine.get_engine()
    tape = eng.tape_for(sdf)

    if bounds is None:
        bounds = _estimate_bounds(sdf)
    (x0, y0, z0), (x1, y1, z1) = bounds

    if x is not None:
        X = np.array([x])
        Y = np.linspace(y0, y1, w)
        Z = np.linspace(z0, z1, h)
        extent = (Z[0], Z[-1], Y[0], Y[-1])
        axes = 'ZY'
    elif y is not None:
        Y = np.array([y])
        X = np.linspace(x0, x1, w)
        Z = np.linspace(z0, z1, h)
        extent = (Z[0], Z[-1], X[0], X[-1])
        axes = 'ZX'
    elif z is not None:
        Z = np.array([z])
        X = np.linspace(x0, x1, w)
        Y = np.linspace(y0, y1, h)
        extent = (Y[0], Y[-1], X[0], X[-1])
        axes = 'YX'
    else:
        raise Exception('x, y, or z position must be specified')

    return eng.eval_grid(tape, X, Y, Z).reshape((w, h)), extent, axes


def show_slice(*args, **kwargs):
    """matplotlib viewer around sample_slice (reference sdf/core.py:234-244)"""
    import matplotlib.pyplot as plt
    show_abs = kwargs.pop('abs', False)
    a, extent, axes = sample_slice(*args, **kwargs)
    if show_abs:
        a = np.abs(a)
    im = plt.imshow(a, extent=extent, origin='lower')
    plt.xlabel(axes[0])
    plt.ylabel(axes[1])
    plt.colorbar(im)
    plt.show()
