"""Parity tests proper: the HIP path (through the C ABI, sdf_amd/engine.py) against the CPU
oracle on the same inputs and against the committed reference goldens.  All need an MI355X."""
import glob
import hashlib
import os

import numpy as np
import pytest

import fixtures
from conftest import GOLDEN, ROOT, value_tolerance
from sdf_amd import core, tape
from sdf_amd.engine import SdfStats
from test_register_slots import files_holding, is_trig

pytestmark = pytest.mark.gpu

# models whose tape contains libm-dependent operations (sin/cos/atan2/hypot/fmod/pow): the device
# libm (ocml) and glibc agree to ~1 ulp, not bitwise
TRIG = {'ex_gearlike', 'ex_weave', 'ex_knurling', 'circular_array', 'twist', 'bend', 'bend_radial',
        'transition_radial', 'wrap_around', 'ease_in_sine', 'ease_out_sine', 'ease_in_out_sine',
        'ease_in_expo', 'ease_out_expo', 'ease_in_out_expo', 'ease_in_elastic', 'ease_out_elastic',
        'ease_in_out_elastic'}


def test_native_library_is_loaded(eng):
    from sdf_amd import engine
    assert os.path.exists(engine.LIB_PATH)
    maps = open('/proc/self/maps').read()
    assert 'libsdf_hip.so' in maps


@pytest.mark.parametrize('name', sorted(fixtures.FIXTURES))
def test_values_match_oracle_and_reference(name, ns, golden_values, oracle_lib, eng):
    P = golden_values['P']
    f = fixtures.build(name, ns)
    v = eng.eval_points(f, P)
    o = oracle_lib.evaluate(f, P)
    ref = golden_values['v_' + name]
    assert np.array_equal(np.isnan(v), np.isnan(o))
    if name in TRIG:
        ok = ~np.isnan(o)
        assert np.all(np.abs(v[ok] - o[ok]) <= value_tolerance(o[ok], P[ok]))
    else:
        assert np.array_equal(v, o, equal_nan=True)       # bit-exact vs the oracle
    ok = ~np.isnan(ref)
    assert np.all(np.abs(v[ok] - ref[ok]) <= value_tolerance(ref[ok], P[ok]))   # vs the reference


def test_call_operator_is_drop_in(ns, golden_values):
    """SDF3.__call__ returns (N,1) float64 like reference sdf/d3.py:24-25"""
    P = golden_values['P']
    f = fixtures.build('ex_example', ns)
    out = f(P)
    assert out.shape == (len(P), 1) and out.dtype == np.float64
    assert np.array_equal(out.reshape(-1), golden_values['v_ex_example'])
    c = ns['circle'](1.2, (0.3, -0.1))
    out2 = c(P[:, :2].copy())
    assert out2.shape == (len(P), 1)


def test_float32_mode_is_close(ns, golden_values, eng):
    from sdf_amd import engine
    P = golden_values['P'][:500]
    f = fixtures.build('ex_example', ns)
    eng.precision = engine.PRECISION_F32
    try:
        v = eng.eval_points(f, P)
    finally:
        eng.precision = engine.PRECISION_F64
    ref = golden_values['v_ex_example'][:500]
    assert np.all(np.abs(v - ref) <= 1e-5 * np.maximum(1.0, np.abs(P).max(axis=1)))


MC = np.load(os.path.join(GOLDEN, 'mc_volumes.npz'))
MC_NAMES = sorted(k[4:] for k in MC.files if k.startswith('vol_'))


@pytest.mark.parametrize('name', MC_NAMES)
def test_marching_cubes_matches_oracle(name, oracle_lib, eng):
    vol = MC['vol_' + name]
    got = eng.marching_cubes(vol)
    want, namb = oracle_lib.marching_cubes(vol)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))      # bit-exact, same order
    ref = MC['soup_' + name]                                              # and equal to skimage
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


MC33 = np.load(os.path.join(GOLDEN, 'mc33_volumes.npz'))
MC33_NAMES = sorted(k[4:] for k in MC33.files if k.startswith('vol_'))


@pytest.mark.parametrize('name', MC33_NAMES)
def test_marching_cubes_lewiner_cases_match_skimage(name, eng):
    """every Lewiner case / subcase / centre vertex (tools/make_golden_mc33.py): skimage's soup bit for bit"""
    got = eng.marching_cubes(MC33['vol_' + name])
    ref = MC33['soup_' + name]
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_marching_cubes_random_volumes(oracle_lib, eng):
    rng = np.random.RandomState(5)
    for shape in [(2, 2, 2), (3, 7, 5), (17, 4, 9), (40, 33, 21), (64, 64, 64)]:
        vol = rng.standard_normal(shape) + rng.uniform(-1, 1)
        got = eng.marching_cubes(vol)
        want, _ = oracle_lib.marching_cubes(vol)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


GEN = sorted(glob.glob(os.path.join(GOLDEN, 'gen_*.npz')))


@pytest.mark.parametrize('path', GEN, ids=[os.path.basename(p)[4:-4] for p in GEN])
def test_generate_matches_oracle_and_reference(path, ns, oracle_lib, eng):
    d = np.load(path)
    name = str(d['fixture'])
    kw = eval(str(d['kwargs']))
    f = fixtures.build(name, ns)
    bounds = tuple(map(tuple, d['bounds']))
    X, Y, Z, _ = core.grid_axes(bounds, d['step'].tolist())
    bs, sparse = kw.get('batch_size', 32), kw.get('sparse', True)
    mesh = eng.generate(f, X, Y, Z, bs, sparse)
    pts, kinds, st = mesh.points(), mesh.kinds(), mesh.stats()
    mesh.close()
    o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
    assert np.array_equal(kinds, d['kinds'])                    # reference classification
    assert np.array_equal(kinds, o.kinds)
    assert (st['skipped'], st['empty'], st['nonempty']) == tuple(int((o.kinds == k).sum()) for k in (0, 1, 2))
    assert st['n_eval_voxels'] == o.n_eval
    if name in TRIG:
        assert pts.shape == o.points.shape
        extent = np.ptp(np.array(bounds), axis=0).max()
        assert np.abs(pts - o.points).max() <= 1e-5 * extent     # north-star tolerance
        assert (pts == o.points).mean() > 0.999
    else:
        assert np.array_equal(pts, o.points)                    # bit-exact, reference order
        assert hashlib.sha256(pts.tobytes()).digest() == d['sha256'].tobytes()   # == reference


@pytest.mark.parametrize('bs', [33, 40, 64, 100])
def test_batch_size_above_32_goes_through_device_memory(bs, ns, oracle_lib, eng):
    """batch_size > 32 (reference sdf/core.py:87, 114-119 takes any): the (batch_size + 1)^3 tile does not fit LDS; the batches
    are sampled into device memory (k_eval_tiles) and marched there (k_field_*): same soup, classification and order as the
    checker's restatement of `generate` -- regular, ragged and single-batch grids, sparse and not, sharded, into a caller
    buffer (reported as not filled, like one that is too small), asynchronously.  The reference's own soups at batch sizes
    40 / 48 / 64 / 128 are the gen_*_b*.npz goldens of test_generate_matches_oracle_and_reference."""
    import torch
    f = fixtures.build('ex_example', ns)
    for samples, sparse in ((2 ** 18, True), (2 ** 20, False), (30000, True)):
        X, Y, Z, _ = core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=samples)
        o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
        m = eng.generate(f, X, Y, Z, bs, sparse)
        st = m.stats()
        assert np.array_equal(m.points(), o.points) and np.array_equal(m.kinds(), o.kinds)
        assert (st['skipped'], st['empty'], st['nonempty']) == tuple(int((o.kinds == k).sum()) for k in (0, 1, 2))
        assert st['n_eval_voxels'] == o.n_eval and st['triangles'] == len(o.points) // 3
        offs = m.batch_offsets()                                 # (r05 advisor: these meshes had no look-back words)
        assert offs[0] == 0 and offs[-1] == len(o.points) // 3 and np.array_equal(np.diff(offs) > 0, o.kinds == 2)
        m.close()
    # shards concatenate to the whole; a caller buffer is not filled but the soup is there; the asynchronous entry point too
    parts = []
    for i in range(3):
        m = eng.generate(f, X, Y, Z, bs, True, shard=(i, 3))
        parts.append(m.points()); m.close()
    assert np.array_equal(np.concatenate(parts), o.points)
    buf = torch.full((9 * (len(o.points) // 3) + 9,), -7.0, dtype=torch.float64, device='cuda:0')
    for wait in (True, False):
        m = eng.generate(f, X, Y, Z, bs, True, out_ptr=buf.data_ptr(), out_cap=len(o.points) // 3, wait=wait)
        assert np.array_equal(m.points(), o.points) and not m.emitted and float(buf[-1]) == -7.0
        m.close()


def test_generate_drop_in_api_and_stl(ns, tmp_path, capsys):
    """f.generate()/f.save() keep the reference signatures, prints and STL bytes"""
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s15.npz'))
    pts = f.generate(samples=2 ** 15, workers=3, batch_size=32, verbose=True, sparse=True)
    out = capsys.readouterr().out
    assert 'min -0.84543' in out and 'batches with 3 workers' in out and 'triangles in' in out
    assert '0 skipped, 0 empty, 1 nonempty' in out
    assert isinstance(pts, np.ndarray) and pts.shape == d['points'].shape
    assert np.array_equal(pts, d['points'])                      # bounds estimated on the device too
    p = str(tmp_path / 'out.stl')
    f.save(p, samples=2 ** 15, verbose=False)
    ref = np.load(os.path.join(GOLDEN, 'stl_example_s15.npz'))['stl'].tobytes()
    assert open(p, 'rb').read() == ref


def test_device_stl_records_match_host_writer(ns, eng):
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s17.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    mesh = eng.generate(f, X, Y, Z)
    rec = mesh.stl_records()
    from sdf_amd import stl
    assert rec.tobytes() == stl.stl_records(mesh.points()).tobytes()
    mesh.close()


def test_bounds_estimated_on_device_match_reference(ns):
    b = np.load(os.path.join(GOLDEN, 'bounds.npz'))
    for name in ('ex_example', 'ex_blobby', 'ex_pawn', 'torus', 'box2', 'capsule', 'smooth_union', 'slice',
                 'extrude_to', 'ex_gearlike', 'ex_weave'):
        got = np.array(core._estimate_bounds(fixtures.build(name, ns)))
        if name in TRIG:
            assert np.allclose(got, b[name], rtol=0, atol=1e-9), name
        else:
            assert np.array_equal(got, b[name]), name


def test_sample_slice(ns, oracle_lib):
    f = fixtures.build('ex_example', ns)
    a, extent, axes = core.sample_slice(f, w=64, h=48, z=0.1, bounds=((-1, -1, -1), (1, 1, 1)))
    assert a.shape == (64, 48) and axes == 'YX'
    Xs, Ys = np.linspace(-1, 1, 64), np.linspace(-1, 1, 48)
    P = np.array([(x, y, 0.1) for x in Xs for y in Ys])
    assert np.array_equal(a.reshape(-1), oracle_lib.evaluate(f, P))
    with pytest.raises(Exception):
        core.sample_slice(f, bounds=((-1, -1, -1), (1, 1, 1)))


def test_sharded_generate_concatenates_to_single(ns, eng):
    """the multi-GPU split (contiguous chunks of the surviving work list) reproduces the
    single-GPU soup when the shards are concatenated in rank order"""
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s22.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    whole = eng.generate(f, X, Y, Z)
    ref = whole.points()
    assert hashlib.sha256(ref.tobytes()).digest() == d['sha256'].tobytes()    # BASELINE config 1
    for world in (2, 3, 8):
        parts, ne, nn = [], 0, 0
        for r in range(world):
            m = eng.generate(f, X, Y, Z, shard=(r, world))
            parts.append(m.points())
            st = m.stats(); ne += st['empty']; nn += st['nonempty']
            k = m.kinds()
            assert set(np.unique(k)) <= {0, 1, 2, 3}
            m.close()
        assert np.array_equal(np.concatenate(parts), ref)
        assert (ne, nn) == (whole.stats()['empty'], whole.stats()['nonempty'])
    whole.close()


def test_edge_cases(ns, eng, oracle_lib):
    f = fixtures.build('ex_example', ns)
    # ragged grids: single-sample trailing slices, non-cubic, tiny
    for shape_step in [((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85), (0.0531, 0.0531, 0.0531)),   # 33 samples: 2 batches/axis, last has 1 sample
                       ((-0.9, -0.4, -0.2), (0.9, 0.5, 0.3), (0.013, 0.05, 0.11)),
                       ((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (0.1, 0.1, 0.1)),                   # one sample per axis
                       ((2.0, 2.0, 2.0), (3.0, 3.0, 3.0), (0.1, 0.1, 0.1))]:                     # nothing there
        lo, hi, step = shape_step
        X, Y, Z, _ = core.grid_axes((lo, hi), step)
        for sparse in (True, False):
            for bs in (32, 7):
                m = eng.generate(f, X, Y, Z, bs, sparse)
                o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
                assert np.array_equal(m.kinds(), o.kinds)
                assert np.array_equal(m.points(), o.points)
                m.close()
    # empty axes
    m = eng.generate(f, np.zeros(0), np.arange(3.0), np.arange(3.0))
    assert m.n_triangles == 0 and m.points().shape == (0, 3)
    # bad arguments fail loudly
    from sdf_amd import engine
    with pytest.raises(engine.SdfHipError):
        eng.generate(f, np.arange(4.0), np.arange(4.0), np.arange(4.0), batch_size=513)
    with pytest.raises(engine.SdfHipError):
        eng.generate(f, np.arange(4.0), np.arange(4.0), np.arange(4.0), batch_size=0)


@pytest.mark.timeout(900)
def test_full_size_config2_properties(ns, eng):
    """BASELINE config 2 (example at 512^3): classification and triangle counts equal the
    reference's measured run, the soup is a closed 2-manifold (every undirected
    edge is used by exactly two triangles, with opposite directions), has no degenerate
    triangle, and is identical across two runs and across precisions' triangle counts"""
    f = fixtures.build('ex_example', ns)
    b = np.load(os.path.join(GOLDEN, 'bounds.npz'))['ex_example']
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, b)), samples=2 ** 27)
    assert (len(X), len(Y), len(Z)) == (512, 512, 512)
    m = eng.generate(f, X, Y, Z)
    st = m.stats()
    assert (st['batches'], st['skipped'], st['empty'], st['nonempty']) == (4096, 2352, 120, 1624)
    assert st['triangles'] == 2945152
    pts = m.points()
    m.close()
    m2 = eng.generate(f, X, Y, Z)
    assert np.array_equal(m2.points(), pts)                      # deterministic, order included
    m2.close()
    tri = pts.reshape(-1, 3, 3)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    assert area2.min() > 0
    verts, inv = np.unique(pts, axis=0, return_inverse=True)
    inv = inv.reshape(-1, 3)
    a = np.concatenate([inv[:, 0], inv[:, 1], inv[:, 2]])
    c = np.concatenate([inv[:, 1], inv[:, 2], inv[:, 0]])
    directed = a.astype(np.int64) * len(verts) + c
    opposite = c.astype(np.int64) * len(verts) + a
    assert len(np.unique(directed)) == len(directed)             # no directed edge twice
    assert np.array_equal(np.sort(directed), np.sort(opposite))  # each edge has its opposite
    # Euler characteristic of a closed orientable surface is even (genus-5 solid here: 2 - 2*5)
    V, E, F = len(verts), len(directed) // 2, len(tri)
    assert V - E + F == 2 - 2 * 5


# BASELINE.json configs at their full sizes: batch classification and triangle counts the
# UNMODIFIED reference produced in the build container (measured by running
# it; the soups themselves are too large to commit).  Bounds come from the device `_estimate_bounds`.
FULL_SIZE = [
    # fixture, samples, (batches, skipped, empty, nonempty), triangles
    ('ex_example', 2 ** 22, (216, 44, 60, 112), 291028),
    ('ex_example', 2 ** 27, (4096, 2352, 120, 1624), 2945152),
    ('ex_gearlike', 2 ** 30, (33856, 26754, 2098, 5004), 10204096),
    ('ex_blobby', 2 ** 30, (32768, 30136, 608, 2024), 4048520),
    ('ex_weave', 2 ** 24, (578, 162, 32, 384), 836368),
]


@pytest.mark.parametrize('name,samples,counts,tris', FULL_SIZE, ids=['%s-2^%d' % (n[3:], s.bit_length() - 1) for n, s, _, _ in FULL_SIZE])
def test_full_size_configs_match_reference_counts(name, samples, counts, tris, ns, eng):
    f = fixtures.build(name, ns)
    bounds = core._estimate_bounds(f)
    X, Y, Z, _ = core.grid_axes(bounds, samples=samples)
    mesh = eng.generate(f, X, Y, Z, 32, True)
    st = mesh.stats()
    assert (st['batches'], st['skipped'], st['empty'], st['nonempty']) == counts
    assert st['triangles'] == tris
    # size-independent properties of the soup: inside the sampled box, finite, reference order
    pts = mesh.points()
    kinds = mesh.kinds()
    mesh.close()
    assert pts.shape == (3 * tris, 3) and np.isfinite(pts).all()
    lo = np.array([X[0], Y[0], Z[0]]); hi = np.array([X[-1], Y[-1], Z[-1]])
    assert (pts >= lo).all() and (pts <= hi).all()
    assert int((kinds == 2).sum()) == counts[3]
    # batches are emitted in X-major batch order: the x batch index of the triangle centroids
    # never decreases along the soup
    cx = pts[:, 0].reshape(-1, 3).mean(axis=1)
    bi = np.minimum(((cx - X[0]) / ((X[1] - X[0]) * 32)).astype(np.int64), (len(X) - 1) // 32)
    assert (np.diff(bi) >= 0).all()


def test_generate_to_device_matches_host_path(ns, eng):
    """sdf_generate_to_device: the in-chain gather into caller device memory gives the same soup as
    the two-step path; a buffer that is too small is reported, not overrun"""
    import torch
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s17.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    ref = eng.generate(f, X, Y, Z)
    want = ref.points()
    ref.close()
    t = len(want) // 3
    buf = torch.full((9 * (t + 5),), -7.0, dtype=torch.float64, device='cuda:0')
    m = eng.generate(f, X, Y, Z, out_ptr=buf.data_ptr(), out_cap=t + 5)
    assert m.emitted and m.n_triangles == t
    eng.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:9 * t].reshape(-1, 3), want)
    assert (got[9 * t:] == -7.0).all()
    m.close()
    # too small by one triangle: reported, nothing written past the capacity (the guard words
    # behind it stay intact), and the mesh still holds the complete soup
    small = torch.full((9 * (t - 1) + 18,), -7.0, dtype=torch.float64, device='cuda:0')
    m = eng.generate(f, X, Y, Z, out_ptr=small.data_ptr(), out_cap=t - 1)
    assert not m.emitted and m.n_triangles == t
    eng.synchronize()
    assert (small.cpu().numpy()[9 * (t - 1):] == -7.0).all()
    assert np.array_equal(m.points(), want)
    m.close()


@pytest.mark.parametrize('driver', ['native', 'native-sharded-skip', 'torch'])
def test_sharded_generate_over_rccl_single_rank(driver, ns, eng, monkeypatch):
    """the multi-GPU code path with a one-rank `nccl` process group must reproduce the plain path bit for bit:
    `native` = the exchange step inside the library (csrc/sdf_comm.hip: ncclAllGather through the dlopen'ed librccl,
    persistent buffers, the default under nccl); `native-sharded-skip` = the same with the skip test shared out and its
    verdicts all-gathered (SDF_SKIP_SHARD_MIN: every grid takes that path); `torch` = sdf_amd/dist.py's protocol through
    torch.distributed (SDF_DIST_NATIVE=0: what other backends and engines use)"""
    import socket
    import torch
    import torch.distributed as td
    from sdf_amd import dist
    monkeypatch.setenv('SDF_DIST_NATIVE', '0' if driver == 'torch' else '1')
    if driver == 'native-sharded-skip':
        monkeypatch.setenv('SDF_SKIP_SHARD_MIN', '0')
    dist.shutdown_native()
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s17.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    ref = eng.generate(f, X, Y, Z)
    want = ref.points()
    ref_kinds = ref.kinds()
    ref.close()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    td.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        tape = eng.tape_for(f)
        for chunks in (1, 1, 2):          # (the second call runs on the capacities the first one learned)
            soup, st = dist.generate_sharded_device(eng, tape, X, Y, Z, 32, True, device=torch.device('cuda', 0), chunks=chunks)
            torch.cuda.synchronize()
            got = soup.cpu().numpy().reshape(-1, 3)
            assert st['triangles'] == len(want) // 3 and st['chunks'] == chunks and st['payload'].startswith('16-byte')
            assert ('native' in st.get('exchange', '')) == (driver != 'torch')
            assert np.array_equal(got, want)
            assert st['ms_mesh'] > 0 and st['ms_exchange'] >= 0 and st['ms_expand'] > 0
            assert (st['batches'], st['skipped'] + st['empty'] + st['nonempty']) == (len(ref_kinds), len(ref_kinds))
        # two steps in flight on lanes of their own (bench.py for N > 1), a different job on each, collected in order
        g = fixtures.build('ex_blobby', ns)
        Xb = np.arange(-4.4, 4.4, 8.8 / 130)
        mb = eng.generate(g, Xb, Xb, Xb)
        want_b = mb.points(); mb.close()
        steps = [dist.submit_sharded(eng, tape, X, Y, Z, 32, True, device=torch.device('cuda', 0), lane=0),
                 dist.submit_sharded(eng, eng.tape_for(g), Xb, Xb, Xb, 32, True, device=torch.device('cuda', 0), lane=1),
                 dist.submit_sharded(eng, tape, X, Y, Z, 32, True, device=torch.device('cuda', 0), lane=0)]
        for step, w in zip(steps, (want, want_b, want)):
            soup, st = dist.collect_sharded(step)
            torch.cuda.synchronize()
            assert np.array_equal(soup.cpu().numpy().reshape(-1, 3), w) and st['triangles'] == len(w) // 3
        pts = f.generate(bounds=tuple(map(tuple, d['bounds'])), step=d['step'].tolist(), verbose=False)
        assert np.array_equal(pts, want)          # core.generate takes the sharded route when dist is up
        # batch_size > 32 is not part of the 16-byte exchange: its soup travels as float64 through torch.distributed, whatever the driver
        big = eng.generate(f, X, Y, Z, 48)
        want48 = big.points(); big.close()
        pts = f.generate(bounds=tuple(map(tuple, d['bounds'])), step=d['step'].tolist(), batch_size=48, verbose=False)
        assert np.array_equal(pts, want48)
    finally:
        dist.shutdown_native()
        td.destroy_process_group()


def test_skip_test_in_pieces_and_generate_from_its_verdicts(ns, eng):
    """what the ranks of a sharded step do between them (csrc/sdf_comm.hip): each runs `_skip` for a share of the
    batches (sdf_skip_kinds), the one-byte verdicts are gathered, and every rank meshes its share of the work list
    from them (sdf_generate_from_kinds).  Here one device plays the three ranks: the assembled verdicts must equal the
    plain call's classification and the soups must be the plain call's, whole and in shards"""
    import torch
    for name, samples in (('ex_example', 2 ** 22), ('ex_gearlike', 2 ** 21), ('ex_blobby', 2 ** 24)):
        f = fixtures.build(name, ns)
        X, Y, Z, _ = core.grid_axes(tuple(map(tuple, BOUNDS[name])), samples=samples)
        m = eng.generate(f, X, Y, Z)
        want, kinds = m.points(), m.kinds()
        m.close()
        nb = len(kinds)
        world = 3
        piece = -(-nb // world)
        buf = torch.full((piece * world,), 77, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        for r in (2, 0, 1):
            eng.skip_kinds(f, X, Y, Z, 32, min(nb, piece * r), min(nb, piece * (r + 1)), buf.data_ptr())
        got = buf.cpu().numpy()
        assert (got[nb:] == 77).all()                                      # nothing outside the grid's batches
        assert np.array_equal(got[:nb] != 0, kinds != 0) and set(np.unique(got[:nb])) <= {0, 255}
        m = eng.generate_from_kinds(f, X, Y, Z, 32, buf.data_ptr())
        assert np.array_equal(m.points(), want) and np.array_equal(m.kinds(), kinds)
        m.close()
        assert np.array_equal(buf.cpu().numpy(), got)                      # the caller's verdicts are read, never written
        parts = []
        for i in range(world):
            m = eng.generate_from_kinds(f, X, Y, Z, 32, buf.data_ptr(), shard=(i, world))
            parts.append(m.points())
            m.close()
        assert np.array_equal(np.concatenate(parts), want)


@pytest.mark.parametrize('driver', ['torch-gloo', 'native-mock-rccl'])
def test_bench_two_ranks_on_one_device_exchange_slabs_between_processes(driver, tmp_path):
    """`python bench.py --gpus 2` the way the driver starts it (no launcher around it: bench.py starts its ranks
    itself), both ranks on THIS device (RCCL refuses two ranks on one GPU, so torch's own collectives go over gloo), the
    slabs kept in device memory.  `torch-gloo`: two real processes run sdf_amd.dist's device side --
    sdf_generate_compact_async into a slab, the all-gather, sdf_expand_slabs on the step's own stream; `native-mock-rccl`:
    the step inside the library (csrc/sdf_comm.hip, what N > 1 runs under nccl) with tests/native/mock_rccl.cpp standing
    in for librccl.  Rank 0's line must carry the reference's soup hash."""
    import json
    import shutil
    import subprocess
    import sys
    env = dict(os.environ, SDF_BENCH_ONE_DEVICE='1', SDF_BENCH_BACKEND='gloo', SDF_BENCH_COMM_DEVICE='cuda')
    if driver == 'native-mock-rccl':
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        mock = str(tmp_path / 'mock_rccl.so')
        subprocess.run([hipcc, '-shared', '-fPIC', '-O2', '-o', mock, os.path.join(ROOT, 'tests', 'native', 'mock_rccl.cpp')],
                       check=True, capture_output=True, timeout=300)
        env.update(SDF_DIST_NATIVE='force', SDF_RCCL_LIB=mock, MOCK_RCCL_SLOT_MB='512')    # (512^3, 2 ranks: 302 MB first-call slabs)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '1',
                        '--full', '--no-cpu-baseline', '--no-other-configs'], env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['parity_check'] is True
    assert rec['config']['triangles'] == 2945152 and rec['exchange']['payload'].startswith('16-byte')
    assert ('native' in rec['exchange']['driver']) == (driver == 'native-mock-rccl')
    assert len(rec['device_ms']['per_rank_mesh']) == 2 and rec['value'] > 0


EDGE_GRIDS = [
    # (nx, ny, nz): ragged last batches (1-sample and 2-sample slices), single-batch and thin grids
    (33, 33, 33), (34, 33, 65), (2, 2, 2), (1, 40, 40), (64, 1, 3), (97, 5, 34), (3, 3, 130),
]


@pytest.mark.parametrize('shape', EDGE_GRIDS, ids=['x'.join(map(str, s)) for s in EDGE_GRIDS])
@pytest.mark.parametrize('sparse', [True, False])
def test_ragged_and_degenerate_grids_match_oracle(shape, sparse, ns, oracle_lib, eng):
    """the reference's batch slicing gives the last batch on an axis 1..33 samples (a 1-sample
    slice makes skimage raise -> an 'empty' batch, reference sdf/core.py:53-56)"""
    f = fixtures.build('ex_example', ns)
    X = -0.9 + 1.8 * np.arange(shape[0]) / max(shape[0] - 1, 1)
    Y = -0.9 + 1.8 * np.arange(shape[1]) / max(shape[1] - 1, 1)
    Z = -0.9 + 1.8 * np.arange(shape[2]) / max(shape[2] - 1, 1)
    mesh = eng.generate(f, X, Y, Z, 32, sparse)
    pts, kinds, st = mesh.points(), mesh.kinds(), mesh.stats()
    mesh.close()
    o = oracle_lib.generate(f, X, Y, Z, 32, sparse)
    assert np.array_equal(kinds, o.kinds)
    assert pts.shape == o.points.shape and np.array_equal(pts, o.points)
    assert st['n_eval_voxels'] == o.n_eval


def test_no_surface_and_empty_inputs(ns, oracle_lib, eng):
    f = fixtures.build('sphere', ns)
    far = np.linspace(5.0, 6.0, 40)                       # entirely outside: every batch skipped
    m = eng.generate(f, far, far, far, 32, True)
    assert m.n_triangles == 0 and m.points().shape == (0, 3) and (m.kinds() == 0).all()
    m.close()
    m = eng.generate(f, far, far, far, 32, False)         # dense: sampled, no crossing -> 'empty'
    assert m.n_triangles == 0 and (m.kinds() == 1).all()
    m.close()
    empty = np.zeros(0)
    m = eng.generate(f, empty, far, far, 32, True)        # np.arange produced nothing on an axis
    assert m.n_triangles == 0 and m.stats()['batches'] == 0
    m.close()
    assert eng.eval_points(f, np.zeros((0, 3))).shape == (0,)
    assert eng.marching_cubes(np.ones((1, 5, 5))).shape == (0, 3)
    assert eng.marching_cubes(np.ones((4, 4, 4))).shape == (0, 3)


TEX = np.load(os.path.join(GOLDEN, 'texture.npz'))


@pytest.mark.parametrize('name', ['frame', 'blobs', 'noise'])
def test_image_leaf_on_device(name, ns, oracle_lib, eng):
    """sampled 2-D field leaf (reference sdf/text.py:65-153) through the tape interpreter: values
    (2-D and extruded) bit-identical to the reference, device bounds and the meshed soup too"""
    from test_oracle import _pictures
    arr, kw = _pictures()[name]
    f = ns['image'](arr, **kw)
    P = TEX['p2_' + name]
    assert np.array_equal(eng.eval_points(f, P), TEX['v2_' + name], equal_nan=True)
    g = f.extrude(0.4)
    P3 = np.concatenate([P, np.linspace(-0.5, 0.5, len(P)).reshape(-1, 1)], axis=1)
    assert np.array_equal(eng.eval_points(g, P3), TEX['v3_' + name], equal_nan=True)
    assert np.array_equal(np.array(core._estimate_bounds(g)), TEX['gen_bounds_' + name])
    pts = g.generate(samples=2 ** 15, verbose=False)
    assert len(pts) // 3 == int(TEX['gen_ntri_' + name])
    assert hashlib.sha256(pts.tobytes()).digest() == TEX['gen_sha_' + name].tobytes()


def test_text_leaf_runs_on_device(ns, eng, oracle_lib, tmp_path):
    """`text(...)`: the glyph raster depends on the FreeType build, so it is checked against the CPU
    checker on the same texture (not against a golden).  The font is the TrueType font Pillow itself
    carries (Aileron Regular, ImageFont.load_default), written to a file: no system font needed."""
    from PIL import ImageFont
    font = str(tmp_path / 'Aileron-Regular.ttf')
    with open(font, 'wb') as fp:
        fp.write(ImageFont.load_default(size=96).font_bytes)
    t = ns['text'](font, 'MI355X', width=4.0, points=96)
    g = t.extrude(0.5)
    rng = np.random.RandomState(3)
    P = rng.uniform(-2.5, 2.5, (2000, 3)) * np.array([1.0, 0.4, 0.2])
    assert np.array_equal(eng.eval_points(g, P), oracle_lib.evaluate(g, P), equal_nan=True)
    w, h = ns['measure_text'](font, 'MI355X', width=4.0)
    assert w == 4.0 and 0 < h < 4.0
    pts = g.generate(samples=2 ** 18, verbose=False)
    assert len(pts) > 3000 and np.isfinite(pts).all()


# ---- interval prepass (csrc/sdf_prune.h): pruned execution must not change a single bit ----

def _random_csg(rng, ns, depth=0):
    """a random tree of the operations that have an interval form, plus a few that do not"""
    r = lambda lo, hi: float(rng.uniform(lo, hi))
    v3 = lambda s: tuple(float(t) for t in rng.uniform(-s, s, 3))
    if depth >= 3 or (depth > 0 and rng.random() < 0.3):
        k = int(rng.integers(0, 10))
        if k == 0: f = ns['sphere'](r(0.2, 0.7), v3(0.6))
        elif k == 1: f = ns['box']((r(0.2, 0.9), r(0.2, 0.9), r(0.2, 0.9)), v3(0.5))
        elif k == 2: f = ns['rounded_box']((r(0.4, 1.0), r(0.4, 1.0), r(0.4, 1.0)), r(0.02, 0.15))
        elif k == 3: f = ns['torus'](r(0.4, 0.8), r(0.05, 0.2))
        elif k == 4: f = ns['capsule'](v3(0.7), v3(0.7), r(0.05, 0.3))
        elif k == 5: f = ns['cylinder'](r(0.1, 0.5))
        elif k == 6: f = ns['plane'](v3(1.0), v3(0.3))
        elif k == 7: f = ns['octahedron'](r(0.3, 0.9))
        elif k == 8: f = ns['rectangle']((r(0.2, 0.8), r(0.2, 0.8)), (r(-0.3, 0.3), r(-0.3, 0.3))).extrude(r(0.2, 1.0))
        else: f = ns['capped_cylinder'](v3(0.6), v3(0.6), r(0.1, 0.3))
        t = int(rng.integers(0, 6))
        if t == 0: f = f.translate(v3(0.6))
        elif t == 1: f = f.rotate(r(0, 3.0), v3(1.0))
        elif t == 2: f = f.scale(r(0.5, 1.5))
        elif t == 3: f = f.orient(v3(1.0))
        elif t == 4: f = f.translate(v3(0.4)).rotate(r(0, 3.0), v3(1.0))
        return f
    kids = [_random_csg(rng, ns, depth + 1) for _ in range(int(rng.integers(2, 5)))]
    op = ns['union' if depth == 0 else ('union', 'union', 'difference', 'difference', 'intersection')[int(rng.integers(0, 5))]]
    k = None if rng.random() < 0.75 else r(0.05, 0.3)
    f = op(*kids, k=k) if k is not None else op(*kids)
    m = int(rng.integers(0, 8))
    if m == 0: f = f.negate() if depth else f
    elif m == 1: f = f.dilate(r(0.01, 0.1))
    elif m == 2: f = f.shell(r(0.02, 0.1))
    elif m == 3: f = f.translate(v3(0.3))
    elif m == 4: f = f.rotate(r(0, 3.0), v3(1.0))
    return f


@pytest.mark.parametrize('seed', range(16))
def test_pruned_generate_is_bit_identical_random_csg(seed, ns, oracle_lib, eng):
    rng = np.random.default_rng(1000 + seed)
    f = _random_csg(rng, ns)
    n = 97 + 7 * (seed % 3)
    X = np.arange(-1.6, 1.6, 3.2 / n); Y = np.arange(-1.5, 1.5, 3.0 / n); Z = np.arange(-1.4, 1.4, 2.8 / n)
    sparse = seed % 2 == 0          # dense: every batch is sampled, i.e. goes through the prepass
    res = []
    for on in (True, False):
        eng.set_prune(on)
        try:
            m = eng.generate(f, X, Y, Z, 32, sparse)
            res.append((m.points(), m.kinds(), m.stats()))
            m.close()
        finally:
            eng.set_prune(True)
    (p1, k1, s1), (p0, k0, s0) = res
    assert s0['n_pruned_instrs'] == 0
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    o = oracle_lib.generate(f, X, Y, Z, 32, sparse)
    assert np.array_equal(k1, o.kinds) and np.array_equal(p1, o.points)


def test_prepass_prunes_the_canonical_example(ns, eng):
    """most batches of the canonical CSG example are decided by part of the tree"""
    f = fixtures.build('ex_example', ns)
    A = np.arange(-1.2, 1.2, 2.4 / 256)
    m = eng.generate(f, A, A, A, 32, True)
    st = m.stats(); p1 = m.points(); kinds = m.kinds(); m_masks = m.prune_masks(); m.close()
    assert st['n_batch_instrs'] > 0 and st['n_pruned_instrs'] > 0.05 * st['n_batch_instrs']
    masks = m_masks[np.isin(kinds, (1, 2))]
    assert masks.shape == (st['empty'] + st['nonempty'], 16) and (masks[:, :8] != 0).any()
    eng.set_prune(False)
    try:
        m = eng.generate(f, A, A, A, 32, True)
        p0 = m.points(); assert m.stats()['n_pruned_instrs'] == 0; m.close()
    finally:
        eng.set_prune(True)
    assert np.array_equal(p1, p0)


# ---- interval forms of circular_array / repeat / bend_linear (sdf_interval.h): the pruned and culled
# execution against the plain one on the same device (same libm), bit for bit ----

def _both_ways(eng, f, X, Y, Z, sparse=True):
    res = []
    for on in (True, False):
        eng.set_prune(on); eng.set_cull(on)
        try:
            m = eng.generate(f, X, Y, Z, 32, sparse)
            res.append((m.points(), m.kinds(), m.stats()))
            m.close()
        finally:
            eng.set_prune(True); eng.set_cull(True)
    return res


@pytest.mark.parametrize('name,samples', [('ex_gearlike', 2 ** 24), ('ex_weave', 2 ** 23), ('ex_knurling', 2 ** 22)])
def test_interval_passes_on_trig_models_are_bit_identical(name, samples, ns, eng):
    f = fixtures.build(name, ns)
    bounds = core._estimate_bounds(f)
    X, Y, Z, _ = core.grid_axes(bounds, samples=samples)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z)
    assert s0['n_pruned_instrs'] == 0 and s0['n_sampled_voxels'] == s0['n_eval_voxels']
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    if True:
        assert s1['n_pruned_instrs'] > (0.1 if name == 'ex_weave' else 0.01) * s1['n_batch_instrs']
        assert s1['n_sampled_voxels'] < 0.8 * s1['n_eval_voxels']


def _random_array_tree(rng, ns):
    r = lambda lo, hi: float(rng.uniform(lo, hi))
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        k = int(rng.integers(0, 4))
        if k == 0: f = ns['sphere'](r(0.1, 0.3))
        elif k == 1: f = ns['rounded_box']((r(0.2, 0.8), r(0.1, 0.4), r(0.1, 0.4)), r(0.01, 0.05))
        elif k == 2: f = ns['capsule']((-r(0.1, 0.4), 0, 0), (r(0.1, 0.4), 0, r(-0.2, 0.2)), r(0.05, 0.15))
        else: f = ns['cylinder'](r(0.05, 0.2)) & ns['slab'](z0=-r(0.1, 0.5), z1=r(0.1, 0.5))
        w = int(rng.integers(0, 11))
        eases = (ns['ease'].linear, ns['ease'].in_out_quad, ns['ease'].out_cubic, ns['ease'].in_out_circ,
                 ns['ease'].in_out_square, ns['ease'].out_bounce, ns['ease'].in_sine)
        e2 = eases[int(rng.integers(0, len(eases)))]
        if w == 10: f = f.wrap_around(-r(0.5, 1.2), r(0.5, 1.2), e=e2)
        elif w == 5: f = f.twist(r(-3.0, 3.0))
        elif w == 6: f = f.bend(r(-2.0, 2.0))
        elif w == 7: f = f.bend_radial(r(0.1, 0.4), r(0.5, 1.0), r(-0.4, 0.4), e2)
        elif w == 8: f = f.transition_linear(ns['sphere'](r(0.2, 0.5)), (0, 0, -r(0.1, 0.5)), (0, 0, r(0.1, 0.5)), e2)
        elif w == 9: f = f.transition_radial(ns['box'](r(0.3, 0.7)), r(0.0, 0.3), r(0.4, 1.0), e2)
        if w == 0:
            f = f.circular_array(int(rng.integers(1, 12)), r(0.0, 1.2))
        elif w == 1:
            e = (ns['ease'].linear, ns['ease'].in_out_quad, ns['ease'].out_cubic, ns['ease'].in_out_circ,
                 ns['ease'].in_out_square, ns['ease'].out_bounce)[int(rng.integers(0, 6))]
            f = f.bend_linear((-r(0.1, 0.5), 0, 0), (r(0.1, 0.5), 0, 0), (0, r(-0.3, 0.3), r(-0.3, 0.3)), e)
        elif w == 2:
            pad = int(rng.integers(0, 2))
            if rng.random() < 0.5:
                f = f.repeat((r(0.5, 1.2), r(0.5, 1.2), 0), padding=pad)
            else:
                f = f.repeat(r(0.6, 1.3), count=int(rng.integers(0, 3)), padding=pad)
        elif w == 3:
            f = f.translate((r(0.2, 0.8), 0, 0)).circular_array(int(rng.integers(2, 9)), 0).repeat((2.0, 2.0, 0), padding=1)
        if rng.random() < 0.5:
            f = f.rotate(r(0, 3.0), (r(-1, 1), r(-1, 1), 1.0)).translate((r(-0.5, 0.5), r(-0.5, 0.5), r(-0.3, 0.3)))
        parts.append(f)
    f = parts[0]
    for g in parts[1:]:
        c = int(rng.integers(0, 4))
        f = (f | g) if c == 0 else ((f - g) if c == 1 else (ns['union'](f, g, k=r(0.05, 0.2)) if c == 2 else (f | g.translate((0.3, 0.2, 0.1)))))
    return f & ns['sphere'](1.45)


@pytest.mark.parametrize('seed', range(24))
def test_interval_passes_with_arrays_and_bends_random(seed, ns, oracle_lib, eng):
    """on / off identity, and the soup against the tree-walking checker: these trees are what reaches the trig (2,4) and
    (4,4) register files of k_mesh (tests/test_register_slots.py) among the random models"""
    rng = np.random.default_rng(7000 + seed)
    f = _random_array_tree(rng, ns)
    n = 93 + 5 * (seed % 4)
    X = np.arange(-1.5, 1.5, 3.0 / n); Y = np.arange(-1.5, 1.5, 3.0 / n) + 0.003; Z = np.arange(-1.5, 1.5, 3.0 / n) - 0.001
    sparse = seed % 3 != 0
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z, sparse=sparse)
    assert s0['n_pruned_instrs'] == 0
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    o = oracle_lib.generate(f, X, Y, Z, 32, sparse)
    assert np.array_equal(k1, o.kinds) and s1['n_eval_voxels'] == o.n_eval
    assert p1.shape == o.points.shape
    if len(p1):                                                     # north-star tolerance (libm on the way)
        assert np.abs(p1 - o.points).max() <= 1e-5 * 3.0
        assert (p1 == o.points).mean() > 0.999


# ---- vertex weld on the device (reference sdf/core.py:160-164: np.unique(points, axis=0, return_inverse=True)) ----

@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 20), ('ex_blobby', 2 ** 18), ('ex_weave', 2 ** 19)])
def test_weld_matches_numpy_unique(name, samples, ns, eng):
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(core._estimate_bounds(f), samples=samples)
    m = eng.generate(f, X, Y, Z, 32, True)
    soup = m.points()
    pts, cells = m.weld()
    pts2, cells2 = m.weld()          # (cached in the mesh)
    m.close()
    want_pts, want_inv = np.unique(soup, axis=0, return_inverse=True)
    assert pts.shape == want_pts.shape and np.array_equal(pts, want_pts)
    assert cells.dtype == np.int64 and np.array_equal(cells, np.asarray(want_inv).reshape(-1, 3))
    assert np.array_equal(pts, pts2) and np.array_equal(cells, cells2)
    assert np.array_equal(pts[cells.reshape(-1)], soup)          # the indexed mesh reproduces the soup
    # a closed surface: Euler characteristic of the welded mesh of the canonical example (genus 5)
    if name == 'ex_example':
        V, F = len(pts), len(cells)
        E = len(np.unique(np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1), axis=0))
        assert V - E + F == 2 - 2 * 5


def test_weld_handles_signed_zeros_and_empty(ns, eng):
    # a soup with coordinates exactly +-0.0: both zeros are one coordinate (NumPy's comparison)
    f = ns['box'](1.0)
    A = np.arange(-1.0, 1.0001, 0.125)
    m = eng.generate(f, A, A, A, 32, False)
    soup = m.points(); pts, cells = m.weld(); m.close()
    want_pts, want_inv = np.unique(soup, axis=0, return_inverse=True)
    assert np.array_equal(pts, want_pts) and np.array_equal(cells.reshape(-1), np.asarray(want_inv).reshape(-1))
    m = eng.generate(ns['sphere'](0.1).translate((5, 5, 5)), A, A, A, 32, False)
    pts, cells = m.weld(); m.close()
    assert pts.shape == (0, 3) and cells.shape == (0, 3)


def test_adopted_soup_gives_the_same_stl_records_and_weld(ns, eng):
    """sdf_mesh_adopt_soup: a float64 soup that already sits in device memory (the gathered soup of a multi-GPU step, here a
    copy of a single-GPU one) gets STL records and the weld from the same device kernels (core.generate with world > 1)"""
    import torch
    f = fixtures.build('ex_example', ns)
    X, Y, Z, _ = core.grid_axes(core._estimate_bounds(f), samples=2 ** 20)
    m = eng.generate(f, X, Y, Z, 32, True)
    t = m.n_triangles
    buf = torch.empty(9 * t, dtype=torch.float64, device='cuda:0')
    m.emit_device(buf.data_ptr())
    eng.synchronize()
    rec, (pts, cells), soup = m.stl_records().copy(), m.weld(), m.points()
    m.close()
    a = eng.adopt_soup(buf.data_ptr(), t)
    try:
        assert a.n_triangles == t
        assert np.array_equal(a.stl_records(), rec)
        pts2, cells2 = a.weld()
        assert np.array_equal(pts2, pts) and np.array_equal(cells2, cells)
        assert np.array_equal(a.points(), soup)
    finally:
        a.close()
    e = eng.adopt_soup(0, 0)           # an empty soup
    assert e.n_triangles == 0 and len(e.stl_records()) == 0
    e.close()


# ---- calls in flight: sdf_generate_to_device_async / sdf_mesh_wait ----

def test_async_generate_matches_sync(ns, eng):
    import torch
    f = fixtures.build('ex_example', ns)
    g = fixtures.build('ex_blobby', ns)
    A = np.arange(-1.2, 1.2, 2.4 / 160)
    B = np.arange(-4.4, 4.4, 8.8 / 130)
    want = []
    for model, ax in ((f, A), (g, B)):
        m = eng.generate(model, ax, ax, ax, 32, True)
        want.append((m.points(), m.kinds(), m.stats())); m.close()
    bufs = [torch.empty(9 * (1 << 20), dtype=torch.float64, device='cuda:0') for _ in range(10)]
    # ten calls in flight on one context (more than its eight slots), two models alternating
    meshes = [eng.generate((f, g)[i % 2], (A, B)[i % 2], (A, B)[i % 2], (A, B)[i % 2], 32, True,
                           out_ptr=bufs[i].data_ptr(), out_cap=bufs[i].numel() // 9, wait=False) for i in range(10)]
    for i, m in reversed(list(enumerate(meshes))):          # collected out of order
        assert m.wait() is True
        p0, k0, s0 = want[i % 2]
        t = m.n_triangles
        assert t == s0['triangles'] and np.array_equal(m.kinds(), k0)
        assert np.array_equal(bufs[i][:9 * t].cpu().numpy().reshape(-1, 3), p0)
        st = m.stats()
        assert (st['skipped'], st['empty'], st['nonempty']) == (s0['skipped'], s0['empty'], s0['nonempty'])
        assert st['ms_mesh'] > 0
        m.close()
    # a buffer that is too small: the call is repeated into library memory, nothing is written past the end
    small = torch.full((9 * 1000 + 9,), -7.0, dtype=torch.float64, device='cuda:0')
    m = eng.generate(f, A, A, A, 32, True, out_ptr=small.data_ptr(), out_cap=1000, wait=False)
    assert m.wait() is False and m.n_triangles == want[0][2]['triangles']
    assert np.array_equal(m.points(), want[0][0]) and float(small[-1]) == -7.0
    m.close()
    # a mesh that is read without wait() collects itself; one that is dropped in flight is harmless
    m = eng.generate(f, A, A, A, 32, True, out_ptr=bufs[0].data_ptr(), out_cap=bufs[0].numel() // 9, wait=False)
    assert m.n_triangles == want[0][2]['triangles']
    m.close()
    m = eng.generate(f, A, A, A, 32, True, out_ptr=bufs[0].data_ptr(), out_cap=bufs[0].numel() // 9, wait=False)
    m.close()
    m = eng.generate(f, A, A, A, 32, True)
    assert np.array_equal(m.points(), want[0][0]); m.close()


def test_async_calls_beyond_the_slot_count_keep_their_own_results(ns, eng):
    """eleven calls in flight on the context's eight call slots, every one a DIFFERENT job (three models on
    eleven grids), collected out of order, with synchronous calls in between: a call that needs the slot of
    an uncollected one collects that mesh first, so every mesh reports its own counters"""
    import torch
    models = [fixtures.build(n, ns) for n in ('ex_example', 'ex_blobby', 'torus')]
    jobs = []
    for i in range(11):
        model = models[i % 3]
        half = (1.2, 4.4, 1.4)[i % 3]
        ax = np.arange(-half, half, 2 * half / (96 + 12 * i))
        jobs.append((model, ax))
    want = []
    for model, ax in jobs:
        m = eng.generate(model, ax, ax, ax, 32, True)
        want.append((m.points(), m.kinds(), m.stats())); m.close()
    assert len({w[2]['triangles'] for w in want}) == 11         # pairwise different results
    bufs = [torch.empty(9 * (1 << 20), dtype=torch.float64, device='cuda:0') for _ in range(11)]
    meshes = []
    for i, (model, ax) in enumerate(jobs):
        meshes.append(eng.generate(model, ax, ax, ax, 32, True, out_ptr=bufs[i].data_ptr(), out_cap=bufs[i].numel() // 9, wait=False))
        if i == 8:      # a synchronous call while nine are in flight: it must not take a held slot's staging
            m = eng.generate(jobs[0][0], jobs[0][1], jobs[0][1], jobs[0][1], 32, True)
            assert m.n_triangles == want[0][2]['triangles']; m.close()
    for i in (3, 0, 6, 10, 1, 8, 5, 2, 9, 4, 7):
        m = meshes[i]
        assert m.wait() is True
        p0, k0, s0 = want[i]
        st = m.stats()
        assert m.n_triangles == s0['triangles'] and st['triangles'] == s0['triangles']
        assert (st['batches'], st['skipped'], st['empty'], st['nonempty']) == (s0['batches'], s0['skipped'], s0['empty'], s0['nonempty'])
        assert st['n_eval_voxels'] == s0['n_eval_voxels'] and st['ms_mesh'] > 0 and st['ms_total'] >= st['ms_mesh']
        assert np.array_equal(m.kinds(), k0)
        assert np.array_equal(bufs[i][:9 * s0['triangles']].cpu().numpy().reshape(-1, 3), p0)
        m.close()


def test_results_land_in_recycled_pinned_memory(ns, eng):
    """large results come back in the library's pinned host blocks (sdf_host_alloc); a block returns to the
    free list when the last view of the array is gone and is handed out again"""
    f = fixtures.build('ex_example', ns)
    A = np.arange(-1.2, 1.2, 2.4 / 200)
    m = eng.generate(f, A, A, A, 32, True)
    p1 = m.points()
    assert p1.nbytes > (1 << 20) and p1.base is not None          # (a view of a pinned block)
    want = p1.copy()
    root = p1
    while isinstance(root.base, np.ndarray):
        root = root.base
    addr = root.base.ptr
    del p1, root
    import gc; gc.collect()
    p2 = m.points()                                               # the same block again
    root = p2
    while isinstance(root.base, np.ndarray):
        root = root.base
    assert root.base.ptr == addr and np.array_equal(p2, want)
    rec = m.stl_records()
    view = p2[:10]
    del p2
    gc.collect()
    assert np.array_equal(view, want[:10])                        # a live view keeps its block
    assert len(rec) == 50 * m.n_triangles
    m.close()


def _random_leaf_tree(rng, ns):
    """booleans of the leaves whose interval forms are compositions of interval steps (sdf_interval.h ia_leaf)"""
    r = lambda lo, hi: float(rng.uniform(lo, hi))
    v3 = lambda s: tuple(float(t) for t in rng.uniform(-s, s, 3))

    def leaf():
        k = int(rng.integers(0, 15))
        if k == 12: f = ns['capped_cone'](v3(0.6), v3(0.6), r(0.15, 0.5), r(0.0, 0.4))
        elif k == 13: f = ns['pyramid'](r(0.5, 1.4)).scale(r(0.6, 1.0))
        elif k == 14:
            n = int(rng.integers(3, 8)); a0 = rng.uniform(0, 6.28)
            f = ns['polygon']([(float(rr * np.cos(a0 + 6.283 * i / n)), float(rr * np.sin(a0 + 6.283 * i / n))) for i, rr in enumerate(rng.uniform(0.4, 1.2, n))]).extrude(r(0.2, 0.9))
        elif k == 0: f = ns['wireframe_box']((r(0.5, 1.2), r(0.5, 1.2), r(0.5, 1.2)), r(0.03, 0.12))
        elif k == 1: f = ns['capped_cylinder'](v3(0.6), v3(0.6), r(0.1, 0.4))
        elif k == 2: f = ns['rounded_cone'](r(0.2, 0.5), r(0.05, 0.3), r(0.4, 1.0))
        elif k == 3: f = ns['ellipsoid']((r(0.4, 1.2), r(0.3, 0.9), r(0.3, 1.0)))
        elif k == 4: f = ns['tetrahedron'](r(0.4, 0.9))
        elif k == 5: f = ns['dodecahedron'](r(0.4, 0.9))
        elif k == 6: f = ns['icosahedron'](r(0.4, 0.9))
        elif k == 7: f = ns['rounded_rectangle'](np.array((r(0.5, 1.4), r(0.4, 1.0))), (r(0.02, 0.2), r(0.02, 0.2), r(0.0, 0.2), r(0.02, 0.15))).extrude(r(0.2, 0.9))
        elif k == 8: f = ns['equilateral_triangle']().scale(r(0.4, 0.8)).extrude(r(0.2, 0.9))
        elif k == 9: f = ns['hexagon'](r(0.3, 0.8)).extrude(r(0.2, 0.9))
        elif k == 10: f = ns['rounded_x'](r(0.5, 1.0), r(0.05, 0.2)).extrude(r(0.2, 0.8))
        else: f = ns['vesica'](r(0.6, 1.0), r(0.1, 0.5)).revolve(r(0.0, 0.4)) if rng.random() < 0.5 else ns['vesica'](r(0.6, 1.0), r(0.1, 0.5)).extrude(r(0.2, 0.8))
        t = int(rng.integers(0, 4))
        if t == 0: f = f.translate(v3(0.5))
        elif t == 1: f = f.rotate(r(0, 3.0), v3(1.0))
        elif t == 2: f = f.orient(v3(1.0)).translate(v3(0.3))
        return f

    f = leaf()
    for _ in range(int(rng.integers(1, 4))):
        g = leaf()
        c = int(rng.integers(0, 5))
        f = (f | g) if c == 0 else ((f - g) if c == 1 else ((f & g) if c == 2 else (ns['union'](f, g, k=r(0.05, 0.25)) if c == 3 else ns['difference'](f, g, k=r(0.05, 0.2)))))
    return f


@pytest.mark.parametrize('seed', range(24))
def test_interval_forms_of_composed_leaves_random(seed, ns, oracle_lib, eng):
    rng = np.random.default_rng(9000 + seed)
    f = _random_leaf_tree(rng, ns)
    n = 95 + 6 * (seed % 3)
    X = np.arange(-1.6, 1.6, 3.2 / n); Y = np.arange(-1.5, 1.5, 3.0 / n) + 0.002; Z = np.arange(-1.4, 1.4, 2.8 / n) - 0.001
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z, sparse=seed % 2 == 0)
    assert s0['n_pruned_instrs'] == 0
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    assert s1['n_sampled_voxels'] < s1['n_eval_voxels'] or s1['n_eval_voxels'] == 0   # (every op of these trees has an interval form)
    o = oracle_lib.generate(f, X, Y, Z, 32, seed % 2 == 0)
    assert np.array_equal(k1, o.kinds) and np.array_equal(p1, o.points)


@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 28), ('ex_blobby', 2 ** 29)])
def test_pruning_over_the_work_list_on_large_grids(name, samples, ns, eng):
    """from 8192 batches on the interval prepass runs behind k_compact, over the surviving batches only
    (k_prune_list): same soup as without the passes, and the tapes did get pruned"""
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(core._estimate_bounds(f), samples=samples)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z)
    assert s1['batches'] >= 8192 and s0['n_pruned_instrs'] == 0 and s1['n_pruned_instrs'] > 0
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)


@pytest.mark.parametrize('name', ['frame', 'blobs', 'noise'])
def test_interval_passes_on_texture_leaf_are_bit_identical(name, ns, oracle_lib, eng):
    """the sampled-field leaf has an interval form too (the texels a box can reach): culled + pruned execution
    against the plain one and against the CPU checker"""
    from test_oracle import _pictures
    arr, kw = _pictures()[name]
    g = ns['image'](arr, **kw).extrude(0.4) - ns['sphere'](0.15).translate((0.2, 0.1, 0.2))
    bounds = core._estimate_bounds(g)
    X, Y, Z, _ = core.grid_axes(bounds, samples=2 ** 19)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, g, X, Y, Z)
    assert s0['n_sampled_voxels'] == s0['n_eval_voxels']
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    assert s1['n_sampled_voxels'] < s1['n_eval_voxels']
    o = oracle_lib.generate(g, X, Y, Z, 32, True)
    assert np.array_equal(k1, o.kinds) and np.array_equal(p1, o.points)


# ---- user-written SDFs (reference README.md:258-295, sdf/d3.py:48-63): closures run on the host, everything
# around them on the device; goldens from the unmodified reference running the SAME user code ----

CUSTOM = np.load(os.path.join(GOLDEN, 'custom.npz'))
# compared to a tolerance instead of bit for bit: the closure calls np.sin / np.cos (NumPy's SIMD libm differs by version),
# resp. the model goes through `rotate` = np.dot in the reference (BLAS kernel selection, <= 4 ulp: VERDICT r01 / tests/test_oracle.py)
CUSTOM_LIBM = {'custom_under_transforms', 'custom_op_over_library'}


@pytest.mark.parametrize('name', sorted(fixtures.CUSTOM_FIXTURES))
def test_user_closures_match_reference(name, ns, eng):
    f = fixtures.build(name, ns)
    P = CUSTOM['P']
    v = f(P.copy())
    assert v.shape == (len(P), 1) and v.dtype == np.float64
    v, ref = v.reshape(-1), CUSTOM['v_' + name]
    assert np.array_equal(np.isnan(v), np.isnan(ref))
    ok = ~np.isnan(ref)
    if name in CUSTOM_LIBM:
        assert np.all(np.abs(v[ok] - ref[ok]) <= value_tolerance(ref[ok], P[ok]))
    else:
        assert np.array_equal(v[ok], ref[ok])
    bounds = core._estimate_bounds(f)
    rb = CUSTOM['bounds_' + name]
    assert np.array_equal(np.array(bounds), rb) if name not in CUSTOM_LIBM else np.allclose(np.array(bounds), rb, rtol=0, atol=1e-9)
    rbt = tuple(map(tuple, rb))
    pts = f.generate(samples=2 ** 17, bounds=rbt, verbose=False)
    want = CUSTOM['pts_' + name]
    assert isinstance(pts, np.ndarray) and pts.shape == want.shape
    if name in CUSTOM_LIBM:
        assert np.abs(pts - want).max() <= 1e-5 * np.ptp(rb, axis=0).max() and (pts == want).mean() > 0.999
    else:
        assert np.array_equal(pts, want)
        assert hashlib.sha256(pts.tobytes()).digest() == CUSTOM['sha_' + name].tobytes()
    st = core.generate.last_stats
    assert st['triangles'] == int(CUSTOM['ntri_' + name]) and st['skipped'] + st['empty'] + st['nonempty'] == st['batches']
    # shards of the surviving work list concatenate to the whole; the dense pass gives the same soup
    X, Y, Z, _ = core.grid_axes(rbt, samples=2 ** 17)
    parts = []
    for r in range(3):
        m = eng.generate(f, X, Y, Z, 32, True, shard=(r, 3))
        parts.append(m.points()); m.close()
    assert np.array_equal(np.concatenate(parts), pts)
    m = eng.generate(f, X, Y, Z, 32, False)
    assert np.array_equal(m.points(), pts) and m.stats()['skipped'] == 0
    m.close()


def test_user_closure_save_and_errors(ns, eng, tmp_path):
    f = fixtures.build('custom_leaf_in_example', ns)
    g = fixtures.build('ex_example', ns)                        # the same model from library leaves only
    p1, p2 = str(tmp_path / 'a.stl'), str(tmp_path / 'b.stl')
    f.save(p1, samples=2 ** 16, verbose=False)
    g.save(p2, samples=2 ** 16, verbose=False)
    assert open(p1, 'rb').read() == open(p2, 'rb').read()       # README's sphere IS the library's sphere
    a, _, _ = core.sample_slice(f, w=32, h=24, z=0.1, bounds=((-1, -1, -1), (1, 1, 1)))
    b, _, _ = core.sample_slice(g, w=32, h=24, z=0.1, bounds=((-1, -1, -1), (1, 1, 1)))
    assert np.array_equal(a, b)

    @ns['sdf3']
    def broken(kind):
        def f(p):
            if kind == 'raise':
                raise KeyError('user bug')
            return np.zeros(len(p) + 1)
        return f
    with pytest.raises(KeyError):
        (broken('raise') & ns['box'](1)).generate(samples=2 ** 12, bounds=((-1, -1, -1), (1, 1, 1)), verbose=False)
    with pytest.raises(ValueError):
        (broken('shape') & ns['box'](1)).generate(samples=2 ** 12, bounds=((-1, -1, -1), (1, 1, 1)), verbose=False)
    with pytest.raises(KeyError):
        broken('raise').generate(samples=2 ** 12, bounds=((-1, -1, -1), (1, 1, 1)), verbose=False)
    # the engine is still usable afterwards
    assert len(g.generate(samples=2 ** 12, verbose=False)) > 0
    # batch_size > 32 with a closure in the model (sdf_generate_field with a row-slot count per tile): the README's sphere IS the
    # library's sphere, whose soup at that batch size is the checker's (test_batch_size_above_32_goes_through_device_memory)
    for bs in (40, 64):
        a = f.generate(samples=2 ** 17, batch_size=bs, verbose=False)
        b = g.generate(samples=2 ** 17, batch_size=bs, verbose=False)
        assert len(a) > 1000 and np.array_equal(a, b)


# ---- the voxel-grid leaf of Mesh.sdf (reference sdf/mesh.py:96-105) ----

GRID3D = np.load(os.path.join(GOLDEN, 'grid3d.npz'))


@pytest.mark.parametrize('name', ['torus', 'two_spheres', 'noise'])
def test_grid_leaf_on_device(name, ns, oracle_lib, eng):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), '..', 'tools'))
    import make_golden_custom as mgc
    from sdf_amd import mesh
    X, Y, Z, A, bg, bb = mgc.grids()[name]
    f = mesh.grid_sdf((X, Y, Z), A, bg, bb)
    P = GRID3D['p_' + name]
    v = eng.eval_points(f, P)
    assert np.array_equal(v, GRID3D['v_' + name]) and np.array_equal(v, oracle_lib.evaluate(f, P))
    g = f.translate((0.05, -0.03, 0.02)) | ns['sphere'](0.2).translate((0, 0, 0.5))
    assert np.array_equal(eng.eval_points(g, P), GRID3D['vc_' + name])
    bounds = core._estimate_bounds(g)
    assert np.array_equal(np.array(bounds), GRID3D['bounds_' + name])
    Xa, Ya, Za, _ = core.grid_axes(bounds, samples=2 ** 17)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, g, Xa, Ya, Za)
    assert np.array_equal(p1, p0) and np.array_equal(k1, k0)
    if name != 'noise':                                          # (random voxels: every group holds a sign change)
        assert s1['n_sampled_voxels'] < 0.8 * s1['n_eval_voxels']    # the leaf has an interval form: groups are culled
    assert np.array_equal(p1, GRID3D['pts_' + name])
    assert hashlib.sha256(p1.tobytes()).digest() == GRID3D['sha_' + name].tobytes()
    o = oracle_lib.generate(g, Xa, Ya, Za, 32, True)
    assert np.array_equal(k1, o.kinds) and np.array_equal(p1, o.points)


# ---- the cheap sweeps over EVERY fixture (all node types, all 34 easings, the example models) ----

BOUNDS = np.load(os.path.join(GOLDEN, 'bounds.npz'))


@pytest.mark.parametrize('name', sorted(BOUNDS.files))
def test_device_bounds_match_reference_for_every_fixture(name, ns):
    """`_estimate_bounds` (reference sdf/core.py:62-82) with the 16^3 probes on the device: all 116 reference bounds"""
    got = np.array(core._estimate_bounds(fixtures.build(name, ns)))
    want = BOUNDS[name]
    if np.array_equal(got, want):
        return
    # libm / BLAS dependent models (device ocml vs glibc, fma or not in np.dot): a probe value within a few ulp of the
    # threshold may fall on the other side, which moves a bound by one probe cell of the LAST round at most
    last_cell = np.ptp(want, axis=0) / 14.0
    assert np.all(np.abs(got - want) <= 1.01 * last_cell + 1e-9), (name, got, want)
    assert name in TRIG or np.allclose(got, want, rtol=0, atol=1e-6 * np.ptp(want, axis=0).max()), name


@pytest.mark.parametrize('name', sorted(n for n in fixtures.FIXTURES if n != 'ex_custbox'))
def test_interval_passes_identity_and_oracle_for_every_fixture(name, ns, oracle_lib, eng):
    """every fixture at samples=2**18: the interval passes on and off give the same soup bit for bit (same
    device, same libm), and that soup is the oracle's (bit for bit, or to the north-star tolerance where the
    model goes through libm)"""
    f = fixtures.build(name, ns)
    bounds = tuple(map(tuple, BOUNDS[name]))
    X, Y, Z, _ = core.grid_axes(bounds, samples=2 ** 18)
    (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z)
    assert s0['n_pruned_instrs'] == 0 and s0['n_sampled_voxels'] == s0['n_eval_voxels']
    assert np.array_equal(k1, k0) and p1.shape == p0.shape and np.array_equal(p1, p0)
    o = oracle_lib.generate(f, X, Y, Z, 32, True)
    assert np.array_equal(k1, o.kinds)
    if name in TRIG:
        assert p1.shape == o.points.shape
        if len(p1):
            assert np.abs(p1 - o.points).max() <= 1e-5 * np.ptp(np.array(bounds), axis=0).max()
            assert (p1 == o.points).mean() > 0.999
    else:
        assert np.array_equal(p1, o.points)


# ---- the multi-GPU exchange unit on ONE device: N "ranks" mesh their shards into slabs of one buffer (what the
# all-gather would assemble), k_expand turns them into the soup ----

@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 22), ('ex_gearlike', 2 ** 21), ('ex_blobby', 2 ** 24), ('ex_weave', 2 ** 22)])
def test_slab_exchange_emulated_ranks(name, samples, ns, eng):
    import torch
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, BOUNDS[name])), samples=samples)
    whole = eng.generate(f, X, Y, Z)
    want, wst = whole.points(), whole.stats()
    whole.close()
    T = len(want) // 3
    nwork = wst['empty'] + wst['nonempty']
    for n in (1, 3, 8, 16):
        cap_items = -(-nwork // n) + 1
        cap_tris = T // n + T // 4 + 4096
        sb = eng.slab_bytes(cap_items, cap_tris)
        buf = torch.zeros(n * sb, dtype=torch.uint8, device='cuda:0')
        out = torch.full((9 * (T + 5),), -7.0, dtype=torch.float64, device='cuda:0')
        torch.cuda.synchronize()
        meshes = [eng.generate_compact(f, X, Y, Z, 32, True, (i, n), buf.data_ptr() + i * sb, cap_items, cap_tris) for i in range(n)]
        eng.expand_slabs([buf.data_ptr() + i * sb for i in range(n)], cap_items, cap_tris, out.data_ptr(), T + 5)
        eng.synchronize()
        heads = buf.view(n, sb)[:, :128].cpu().numpy().view(np.int64).reshape(n, 16)
        assert not heads[:, 2].any()                                        # no overflow
        assert int(heads[:, 0].sum()) == T and int(heads[:, 1].sum()) == nwork
        assert (int(heads[:, 3].sum()), int(heads[:, 4].sum())) == (wst['empty'], wst['nonempty'])
        assert int(heads[:, 5].sum()) == wst['n_eval_voxels'] and (heads[:, 9] == nwork).all()
        got = out.cpu().numpy()
        assert np.array_equal(got[:9 * T].reshape(-1, 3), want)             # bit for bit, reference order
        assert (got[9 * T:] == -7.0).all()
        for i, m in enumerate(meshes):
            m.wait()
            assert m.n_triangles == int(heads[i, 0])                         # (the soup itself is in the slab, not in the mesh)
            m.close()
    # slabs that are too small are flagged and never overrun: guard bytes behind every slab stay intact
    n, cap_items, cap_tris = 2, 3, 100
    sb = eng.slab_bytes(cap_items, cap_tris)
    buf = torch.full((n * (sb + 64),), 0x5A, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    meshes = [eng.generate_compact(f, X, Y, Z, 32, True, (i, n), buf.data_ptr() + i * (sb + 64), cap_items, cap_tris) for i in range(n)]
    eng.synchronize()
    b = buf.cpu().numpy().reshape(n, sb + 64)
    assert (b[:, sb:] == 0x5A).all()
    heads = np.ascontiguousarray(b[:, :128]).view(np.int64).reshape(n, 16)
    assert (heads[:, 2] != 0).all() and int(heads[:, 0].sum()) == T        # flagged, and the true counts are reported
    for m in meshes:
        m.close()


def _synthetic_slabs(eng, rng, n, cap_items, cap_tris, sizes_of):
    """n slabs in the layout of csrc/sdf_slab.h (header | prefix words | transforms | 16-byte triangle records | raw area)
    written by NumPy (sdf_amd/slabcodec.py), and the float64 soup `points * scale + offset` (reference sdf/core.py:58-60)
    they expand to.  The triangles have marching cubes' shape (vertices on the edges of one cell); ~ 0.4 % do not (a vertex
    inside a cell) and travel raw"""
    from sdf_amd import slabcodec as sc
    sb = eng.slab_bytes(cap_items, cap_tris)
    L = sc.layout(cap_items, cap_tris)
    assert L['bytes'] == sb
    host = np.zeros((n, sb), np.uint8)
    want = [np.zeros((0, 9))]
    for s in range(n):
        sizes = sizes_of(s)
        ni, nt = len(sizes), int(sizes.sum())
        assert ni <= cap_items and nt <= cap_tris
        host[s, L['prefix_off']:L['prefix_off'] + ni * 8] = (np.cumsum(sizes).astype(np.uint64) | np.uint64(2 << 62)).view(np.uint8)
        xf = rng.uniform(-1, 1, (ni, 6))
        xf[:, 3:] = rng.uniform(0.01, 0.02, (ni, 3))
        host[s, L['xf_off']:L['xf_off'] + ni * 48] = xf.reshape(-1).view(np.uint8)
        c = rng.integers(0, 32, (nt, 3))
        tri = np.zeros((nt, 3, 3), np.float32)
        rows = np.arange(nt)
        for k in range(3):
            v = (c + rng.integers(0, 2, (nt, 3))).astype(np.float32)
            frac = rng.integers(0, 3, nt)
            v[rows, frac] = (c[rows, frac] + rng.random(nt)).astype(np.float32)
            tri[:, k, :] = v
        tri = tri.reshape(nt, 9)
        inside = rng.random(nt) < 0.004
        if nt:
            inside[int(rng.integers(0, nt))] = True         # (at least one raw triangle per non-empty slab)
        tri[inside] = rng.uniform(0, 32, (int(inside.sum()), 9)).astype(np.float32)
        n_raw = sc.write_triangles(host[s], cap_items, cap_tris, tri)
        head = np.zeros(16, np.int64)
        head[0], head[1], head[10], head[11] = nt, ni, n_raw, nt
        host[s, :128] = head.view(np.uint8)
        item = np.repeat(np.arange(ni), sizes)
        want.append(tri.astype(np.float64) * np.tile(xf[item, 3:], 3) + np.tile(xf[item, :3], 3))
    return host, np.concatenate(want)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 8, 64])
def test_expand_synthetic_slabs(n, eng):
    """k_expand alone against NumPy: slabs of random work items (empty items, empty slabs, items of one triangle and of
    thousands), so that workgroups of 256 output triangles straddle items and slabs in every way -- in particular into
    the LAST slab, the case a compiler option once broke (sdf_amd/csrc/sdf_plain.hip)"""
    import torch
    rng = np.random.default_rng(100 + n)
    for scale in (1, 40, 700):
        def sizes_of(s):
            k = int(rng.integers(0, 60)) if s != n - 1 else int(rng.integers(1, 60))
            z = rng.integers(0, scale * 3, k)
            z[rng.random(k) < 0.3] = 0
            return z.astype(np.int64)
        cap_items, cap_tris = 64, 64 * scale * 3
        host, want = _synthetic_slabs(eng, rng, n, cap_items, cap_tris, sizes_of)
        T, sb = len(want), host.shape[1]
        buf = torch.from_numpy(host.reshape(-1)).to('cuda:0')
        for cap_out in (T + 5, max(T - 300, 0)):                               # (a soup that is too small is filled and not overrun)
            out = torch.full((9 * (T + 5),), -7.0, dtype=torch.float64, device='cuda:0')
            torch.cuda.synchronize()
            eng.expand_slabs([buf.data_ptr() + i * sb for i in range(n)], cap_items, cap_tris, out.data_ptr(), cap_out)
            eng.synchronize()
            got = out.cpu().numpy()
            m = min(T, cap_out)
            assert np.array_equal(got[:9 * m].reshape(-1, 9), want[:m])
            assert (got[9 * m:] == -7.0).all()


def test_estimate_bounds_failure_is_numpys(ns):
    """a model no probe of the +-1e9 cube comes near: the reference dies in `where.max(axis=0)` of an empty array
    (reference sdf/core.py:80); so does the device loop, with the same exception type"""
    far = ns['sphere'](1).translate((1e12, 0, 0))
    with pytest.raises(ValueError):
        core._estimate_bounds(far)
    # (and a model with a user closure takes the reference's host loop around the hybrid evaluation)
    f = fixtures.build('custom_leaf_in_example', ns)
    assert np.array_equal(np.array(core._estimate_bounds(f)), CUSTOM['bounds_custom_leaf_in_example'])


def test_bounds_exchange_words_survive_the_tag_wrapping():
    """k_estimate_bounds_w's waves exchange a word per round that carries the CALL's 16-bit tag instead of being zeroed per call
    (csrc/sdf_bounds.hip); the host clears the words when the tag wraps.  A context whose first tag is 65530 (SDF_BOUNDS_TAG0) runs
    through the wrap: the same bounds before, at and after it, for two models in turn (stale words of the other model under every tag)"""
    import subprocess
    import sys
    script = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
import sdf_amd, fixtures
from sdf_amd import core
ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
B = np.load(os.path.join(%r, 'bounds.npz'))
fs = [(n, fixtures.build(n, ns)) for n in ('ex_example', 'ex_blobby', 'torus')]
for rep in range(12):
    for n, f in fs:
        assert np.array_equal(np.array(core._estimate_bounds(f)), B[n]), (rep, n)
print('ok')
''' % (ROOT, ROOT, GOLDEN)
    r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, SDF_BOUNDS_TAG0='65530'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


# ---- the two meshing schemes (one kernel with look-back + parking / sample + number + emit) give the same soup ----

@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 22), ('ex_gearlike', 2 ** 22), ('ex_blobby', 2 ** 23), ('ex_weave', 2 ** 22),
                                          ('ex_knurling', 2 ** 21), ('ex_pawn', 2 ** 21), ('ex_custbox', 2 ** 18), ('wireframe_box', 2 ** 18)])
def test_one_pass_and_two_pass_meshing_agree(name, samples, ns, eng):
    import torch
    f = fixtures.build(name, ns)
    if name == 'ex_custbox':
        bounds = ((-7.0, -4.0, -0.5), (7.0, 4.0, 2.5))
    else:
        bounds = tuple(map(tuple, BOUNDS[name]))
    X, Y, Z, _ = core.grid_axes(bounds, samples=samples)
    res = []
    try:
        for mode in (0, 1):
            eng.set_twopass(mode)
            for sparse in (True, False):
                m = eng.generate(f, X, Y, Z, 32, sparse)
                res.append((mode, sparse, m.points(), m.kinds(), m.stats(), m.batch_offsets()))
                m.close()
            # a caller buffer that is too small: flagged, repeated into library memory, guard intact
            t = res[-2][4]['triangles']
            if t > 10:
                small = torch.full((9 * (t // 2) + 9,), -7.0, dtype=torch.float64, device='cuda:0')
                m = eng.generate(f, X, Y, Z, 32, True, out_ptr=small.data_ptr(), out_cap=t // 2)
                assert not m.emitted and m.n_triangles == t and np.array_equal(m.points(), res[-2][2])
                assert float(small[-1]) == -7.0
                m.close()
    finally:
        eng.set_twopass(-1)
    for sparse in (True, False):
        a = [r for r in res if r[0] == 0 and r[1] == sparse][0]
        b = [r for r in res if r[0] == 1 and r[1] == sparse][0]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[5], b[5])
        for k in ('triangles', 'skipped', 'empty', 'nonempty', 'n_eval_voxels', 'n_ambiguous_cells', 'n_sampled_voxels', 'n_pruned_instrs'):
            assert a[4][k] == b[4][k], k


def test_two_pass_meshing_full_size_and_slabs(ns, oracle_lib, eng):
    """the two-pass scheme at BASELINE config 2: the reference's soup hash; and as the source of exchange slabs"""
    import torch
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'full_c2_example_s27.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    eng.set_twopass(1)
    try:
        m = eng.generate(f, X, Y, Z)
        pts = m.points(); m.close()
        assert hashlib.sha256(pts.tobytes()).digest() == d['sha256'].tobytes()
        T, n = len(pts) // 3, 3
        cap_items, cap_tris = 1744 // n + 2, T // n + T // 4
        sb = eng.slab_bytes(cap_items, cap_tris)
        buf = torch.zeros(n * sb, dtype=torch.uint8, device='cuda:0')
        out = torch.empty(9 * T, dtype=torch.float64, device='cuda:0')
        torch.cuda.synchronize()
        meshes = [eng.generate_compact(f, X, Y, Z, 32, True, (i, n), buf.data_ptr() + i * sb, cap_items, cap_tris) for i in range(n)]
        eng.expand_slabs([buf.data_ptr() + i * sb for i in range(n)], cap_items, cap_tris, out.data_ptr(), T)
        eng.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(-1, 3), pts)
        for mm in meshes:
            mm.close()
    finally:
        eng.set_twopass(-1)


def test_integration_md_bindings_work_as_written():
    """INTEGRATION.md sections 2 / 2b (the reference-side ctypes bindings) as a program: tools/integration_check.py"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(GOLDEN))
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'integration_check.py')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'bindings ok' in out.stdout


# ---- float32: the evaluation entry points keep it, the meshing path does not (round 5) ----

def test_float32_meshing_is_refused(ns, eng):
    """`SDF_PRECISION_F32` sampling of the meshing path was a diagnostic until r04 -- 3.1e-5 (C2) / 1.2e-4 (C3) of the extent at its
    maximum against north_star's 1e-5, and 3.6 x slower than float64 because the interval passes bound the float64 interpreter
    only -- and was removed: `sdf_generate*` refuse it loudly, `sdf_eval_*` / `sdf_estimate_bounds` keep both precisions
    (test_float32_mode_is_close)."""
    from sdf_amd import engine
    f = fixtures.build('ex_example', ns)
    X, Y, Z, _ = core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=2 ** 15)
    eng.precision = engine.PRECISION_F32
    try:
        with pytest.raises(engine.SdfHipError, match='float64'):
            eng.generate(f, X, Y, Z)
        with pytest.raises(engine.SdfHipError, match='float64'):
            eng.generate(f, X, Y, Z, batch_size=40)
        v = eng.eval_points(f, np.zeros((4, 3)))          # (still served)
        assert v.shape == (4, 1) or v.shape == (4,)
    finally:
        eng.precision = engine.PRECISION_F64
    m = eng.generate(f, X, Y, Z)
    assert m.n_triangles > 0
    m.close()


def test_block_scan_of_the_kernels_on_device(tmp_path):
    """block_exclusive_scan (csrc/sdf_device.h: data-parallel-primitive shifts inside the wave, wave totals through LDS)
    against a serial prefix sum, 1024 threads; built from tests/native/scan_check.hip with hipcc"""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'scan_check')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-result', '-I', os.path.join(ROOT, 'sdf_amd', 'csrc'),
                    '-o', exe, os.path.join(ROOT, 'tests', 'native', 'scan_check.hip')], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'bad=0' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 24), ('ex_weave', 2 ** 22), ('ex_blobby', 2 ** 23), ('ex_pawn', 2 ** 23)])
def test_tail_of_the_work_list_by_cost_or_in_order_same_soup(name, samples, ns, eng):
    """k_mesh hands the last (workgroups - 1) surviving batches out by descending cost estimate (MeshArgs::order,
    sdf_ctx_set_tail_order); in list order the soup, the per-batch offsets and the statistics must be the same, in both
    meshing schemes, and small grids (fewer batches than workgroups) must take either path"""
    f = fixtures.build(name, ns)
    bounds = tuple(map(tuple, BOUNDS[name]))
    res = {}
    try:
        for smp in (samples, 2 ** 16):
            X, Y, Z, _ = core.grid_axes(bounds, samples=smp)
            for mode in (0, 1):
                eng.set_twopass(mode)
                for on in (1, 0):
                    eng.set_tail_order(on)
                    m = eng.generate(f, X, Y, Z, 32, True)
                    res[(smp, mode, on)] = (m.points(), m.kinds(), m.batch_offsets(), m.stats())
                    m.close()
    finally:
        eng.set_twopass(-1)
        eng.set_tail_order(1)
    for (smp, mode, on), r in res.items():
        ref = res[(smp, 0, 0)]
        assert np.array_equal(r[0], ref[0]) and np.array_equal(r[1], ref[1]) and np.array_equal(r[2], ref[2]), (smp, mode, on)
        for k in ('triangles', 'skipped', 'empty', 'nonempty', 'n_eval_voxels', 'n_ambiguous_cells', 'n_sampled_voxels', 'n_pruned_instrs'):
            assert r[3][k] == ref[3][k], (smp, mode, on, k)
    assert res[(samples, 0, 0)][3]['triangles'] > 1000


def test_rare_paths_of_the_one_kernel_scheme_on_a_lattice_of_small_spheres(ns, oracle_lib, eng):
    """k_mesh's rarely taken branches in one job (the round-4 advisor asked for it): a lattice of small spheres puts > 2048 surface
    cells and more triangles than the LDS list holds into most tiles -- the per-row counting, the list rebuilt in passes, dense
    tiles (too many units for a slot) next to sparse ones at the lattice's edge (a dense tile takes the slots' region: the waiting
    batch is written first, the work item carried over), batches written right behind their counting next to deferred ones,
    the park slots in use -- with the tail of the list in cost order and in list order, deferred and not, two and three interval
    levels: every soup equal to the checker's, bit for bit."""
    f = ns['sphere'](0.055).repeat(0.17) & ns['box'](1.7)
    X, Y, Z, _ = core.grid_axes(((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), samples=2 ** 23)      # 203^3: 343 batches, ragged far tiles
    o = oracle_lib.generate(f, X, Y, Z, 32, True)
    assert len(o.points) // 3 > 400000
    res = []
    try:
        eng.set_twopass(0)
        for defer, levels, tail in ((1, 0, 1), (1, 0, 0), (0, 0, 1), (1, 3, 1), (1, 2, 0)):
            eng.set_defer(defer); eng.set_cull_levels(levels); eng.set_tail_order(tail)
            m = eng.generate(f, X, Y, Z, 32, True)
            res.append(((defer, levels, tail), m.points(), m.kinds(), m.stats()))
            m.close()
        eng.set_twopass(1)
        m = eng.generate(f, X, Y, Z, 32, True)
        res.append(('two-pass', m.points(), m.kinds(), m.stats()))
        m.close()
    finally:
        eng.set_twopass(-1); eng.set_defer(1); eng.set_cull_levels(0); eng.set_tail_order(1)
    per_tile = max(r[3]['triangles'] for r in res) / max(1, res[0][3]['nonempty'])
    assert per_tile > 3000, per_tile            # (the list of a dense tile holds ~ 2400 entries: passes are needed)
    for key, pts, kinds, st in res:
        assert np.array_equal(kinds, o.kinds), key
        assert np.array_equal(pts, o.points), key


@pytest.mark.parametrize('name,samples', [('ex_example', 2 ** 24), ('ex_example', 1500000), ('ex_blobby', 2 ** 23), ('ex_gearlike', 2 ** 22),
                                          ('ex_weave', 2 ** 22), ('ex_knurling', 2 ** 21), ('ex_pawn', 2 ** 22)])
def test_sparse_tiles_deferred_emission_and_interval_levels_same_soup(name, samples, ns, eng):
    """the one-kernel scheme's choices -- sparse tiles + deferred emission or dense tiles + parking (sdf_ctx_set_defer), two or
    three interval levels in k_cull (sdf_ctx_set_cull_levels; by default the tape decides) -- give the same soup, the same
    per-batch offsets and verdicts bit for bit, on regular and ragged grids, one call at a time and with the tail of the work
    list in order; fewer samples go through the interpreter with three levels than with two"""
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, BOUNDS[name])), samples=samples)
    res = {}
    try:
        eng.set_twopass(0)
        for defer in (1, 0):
            for levels in (0, 2, 3):
                eng.set_defer(defer); eng.set_cull_levels(levels)
                m = eng.generate(f, X, Y, Z, 32, True)
                res[(defer, levels)] = (m.points(), m.kinds(), m.batch_offsets(), m.stats())
                m.close()
        eng.set_defer(1); eng.set_cull_levels(0); eng.set_tail_order(0)
        m = eng.generate(f, X, Y, Z, 32, True)
        res[(1, -1)] = (m.points(), m.kinds(), m.batch_offsets(), m.stats())
        m.close()
    finally:
        eng.set_twopass(-1); eng.set_defer(1); eng.set_cull_levels(0); eng.set_tail_order(1)
    ref = res[(0, 2)]
    assert ref[3]['triangles'] > 1000
    for key, r in res.items():
        assert np.array_equal(r[0], ref[0]) and np.array_equal(r[1], ref[1]) and np.array_equal(r[2], ref[2]), key
        for k in ('triangles', 'skipped', 'empty', 'nonempty', 'n_eval_voxels', 'n_ambiguous_cells', 'n_pruned_instrs'):
            assert r[3][k] == ref[3][k], (key, k)
    for defer in (1, 0):
        assert res[(defer, 3)][3]['n_sampled_voxels'] < res[(defer, 2)][3]['n_sampled_voxels']
        assert res[(defer, 0)][3]['n_sampled_voxels'] in (res[(defer, 2)][3]['n_sampled_voxels'], res[(defer, 3)][3]['n_sampled_voxels'])
    assert res[(1, 3)][3]['n_sampled_voxels'] == res[(0, 3)][3]['n_sampled_voxels']


def test_no_parking_and_tail_by_cost_do_not_wait_for_each_other():
    """With parking off (SDF_PARK=0) EVERY batch waits for its predecessors' counts before it emits -- the case the
    bound `tail <= workgroups - 1` on the reordered tail of the work list is there for ("The end of the
    kernel").  A fresh process (the switch is read when the context is created) meshes three grids in both orders of
    the tail (at these sizes the tail is the whole work list); the soups must be the reference's (gen_* goldens) and the
    process must come back."""
    import subprocess
    import sys
    script = r'''
import os, sys, hashlib
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
import sdf_amd, fixtures
from sdf_amd import core, engine
ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
eng = engine.get_engine(0)
for name in ('gen_example_s22', 'gen_blobby_s20', 'gen_example_s17'):
    d = np.load(os.path.join(%r, name + '.npz'))
    f = fixtures.build(str(d['fixture']), ns)
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    for on in (1, 0):
        eng.set_tail_order(on)
        m = eng.generate(f, X, Y, Z, 32, True)
        sha = hashlib.sha256(m.points().tobytes()).hexdigest()
        m.close()
        assert sha == bytes(d['sha256']).hex(), (name, on)
print('ok')
''' % (ROOT, ROOT, GOLDEN)
    r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, SDF_PARK='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_failed_allocations_leak_nothing():
    """Error paths hand back what they took: the library's test hook (sdf_test_fail_alloc) makes the n-th allocation
    fail inside sdf_ctx_create, sdf_tape_create / sdf_tape_set_prune_info and sdf_generate in turn; every call must
    fail with the allocator's message (never crash), the context must stay usable, and a SECOND round of the same
    failures must leave the device's free memory (hipMemGetInfo) where the first round left it -- a leak on an error
    path would show up once per failure.  (Not compared with the state before the first round: the HIP runtime keeps
    what it allocates on first use -- code objects, a scratch pool per hardware queue: 160 MiB each here.)  A fresh
    process: the hook and the library's buffer pools are process-wide."""
    import subprocess
    import sys
    script = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
import sdf_amd, fixtures
from sdf_amd import core, engine, tape
lib = engine.load_library()
def free():
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value
def err():
    return (lib.sdf_last_error() or b'').decode()
ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
f = fixtures.build('ex_example', ns)
t = tape.lower(f)
X, Y, Z, _ = core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=2 ** 20)
eng0 = engine.Engine(0); dt0 = engine.DeviceTape(eng0, t)
m = eng0.generate(dt0, X, Y, Z); want = m.points().copy(); m.close()
dt0._fin(); eng0._fin()

def one_round():
    n_ctx = 0
    for n in range(1, 10):                                   # ---- sdf_ctx_create ----
        lib.sdf_test_fail_alloc(n)
        h = ctypes.c_void_p()
        rc = lib.sdf_ctx_create(0, ctypes.byref(h))
        lib.sdf_test_fail_alloc(0)
        if rc == 0:
            assert lib.sdf_ctx_destroy(h) == 0
            break
        n_ctx += 1
        assert 'emory' in err(), err()
        assert h.value is None
    assert n_ctx >= 2, n_ctx
    eng = engine.Engine(0)
    n_tape = 0
    for n in range(1, 10):                                   # ---- the tape (sdf_tape_create, sdf_tape_set_prune_info) ----
        lib.sdf_test_fail_alloc(n)
        try:
            dt = engine.DeviceTape(eng, t)
            lib.sdf_test_fail_alloc(0)
            break
        except engine.SdfHipError as e:
            lib.sdf_test_fail_alloc(0)
            n_tape += 1
            assert 'emory' in str(e), e
    assert n_tape >= 4, n_tape
    m = eng.generate(dt, X, Y, Z); assert np.array_equal(m.points(), want); m.close()
    n_gen = 0
    for n in range(1, 40):                                   # ---- sdf_generate: a fresh context has every buffer to allocate ----
        eng2 = engine.Engine(0)
        dt2 = engine.DeviceTape(eng2, t)
        lib.sdf_test_fail_alloc(n)
        try:
            m = eng2.generate(dt2, X, Y, Z)
            lib.sdf_test_fail_alloc(0)
            assert np.array_equal(m.points(), want)
            m.close(); done = True
        except engine.SdfHipError as e:
            lib.sdf_test_fail_alloc(0)
            n_gen += 1; done = False
            assert 'emory' in str(e), e
            m = eng2.generate(dt2, X, Y, Z)                  # the context is still good
            assert np.array_equal(m.points(), want)
            m.close()
        dt2._fin(); eng2._fin()
        if done:
            break
    assert n_gen >= 5, n_gen
    dt._fin(); eng._fin()
    return n_ctx, n_tape, n_gen

first = one_round()
f1 = free()
second = one_round()
f2 = free()
assert first == second and abs(f2 - f1) <= (8 << 20), (first, second, f1, f2)
print('ok', first, f1, f2)
''' % (ROOT, ROOT)
    r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().startswith('ok'), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize('count', [3, 7, 16, 24, 360])
def test_circular_array_at_and_around_sector_boundaries(count, ns, oracle_lib, eng):
    """circular_array in float64 is evaluated in rotation form (csrc/sdf_interp.h L_CIRC_PREP: the sector by a binary search
    of rotations, no atan2 / sin / cos; CIRC_SET: four products) instead of the reference's hypot / arctan2 %% da / cos, sin
    (reference sdf/d3.py:379-392).  The points where the two could part: ON the sector boundaries (angles k * da as exactly
    as float64 has them), one ulp to 1e-9 rad either side, the negative x axis with y = +0 / -0 (arctan2 = +pi / -pi), the
    axis x = y = 0, tiny and huge radii -- tests/golden/circ_boundaries.npz, produced by RUNNING the reference on them
    (tools/make_golden_circ.py).  The children are symmetric about the x axis, so the reference's value is continuous across
    a boundary: whichever sector a last-bit difference of the arctangent picks, the values must agree to the tolerance of
    the libm models -- with the reference AND with the checker; twist and bend (the other users of the inline sin / cos)
    ride along."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_circ as mgc
    g = np.load(os.path.join(GOLDEN, 'circ_boundaries.npz'))
    P = g['P_%d' % count]
    for i, f in enumerate(mgc.models(ns, count)):
        v = eng.eval_points(f, P)
        ref = g['v_%d_%d' % (count, i)]
        o = oracle_lib.evaluate(f, P)
        ok = np.isfinite(ref)
        assert np.array_equal(np.isfinite(v), ok)
        for want in (ref, o):
            assert np.all(np.abs(v[ok] - want[ok]) <= value_tolerance(want[ok], P[ok])), (i, float(np.max(np.abs(v[ok] - want[ok]) / value_tolerance(want[ok], P[ok]))))


@pytest.mark.parametrize('count', [2, 3, 4, 7, 8, 12, 16, 24, 100, 360])
def test_circular_array_on_the_axes_under_asymmetric_children(count, ns, oracle_lib, eng):
    """Points ON the coordinate axes (x == 0.0 or y == +-0.0 exactly: whole planes of a grid like np.arange(-1, 1, 0.01)):
    arctan2 is exact there and so is the reference's floored modulo (sdf/d3.py:381-383), i.e. the reference puts such a point
    into ONE definite sector -- angle 0.0 exactly where da divides the angle in floating point (4 | count) -- and a child that
    is not symmetric about the x axis tells the sectors apart.  The rotation search alone landed ~6e-17 rad on the other side
    for y < 0 (round-4 advisor finding; symmetric children hid it); axis lanes now take the reference's expression
    (csrc/sdf_interp.h L_CIRC_PREP).  Goldens: the unmodified reference on these points, tests/golden/circ_axes.npz
    (tools/make_golden_circ.py); generic points ride along; the whole model also goes through the meshing kernel's
    interpreter variants via eval_points' register files."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_circ as mgc
    g = np.load(os.path.join(GOLDEN, 'circ_axes.npz'))
    P = g['P_%d' % count]
    for i, f in enumerate(mgc.asym_models(ns, count)):
        v = eng.eval_points(f, P)
        ref = g['v_%d_%d' % (count, i)]
        o = oracle_lib.evaluate(f, P)
        for want in (ref, o):
            assert np.all(np.abs(v - want) <= value_tolerance(want, P)), (i, int(np.argmax(np.abs(v - want) / value_tolerance(want, P))), float(np.max(np.abs(v - want) / value_tolerance(want, P))))


def _native_exchange_worker(rank, world, port, q, mock, skip_shard, first_cap):
    import hashlib
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), SDF_RCCL_LIB=mock, SDF_DIST_NATIVE='force')
    if skip_shard:
        os.environ['SDF_SKIP_SHARD_MIN'] = '0'
    if first_cap:
        os.environ['SDF_COMM_FIRST_CAP_TRIS'] = str(first_cap)
    try:
        import torch
        import torch.distributed as td
        torch.cuda.set_device(0)
        td.init_process_group('gloo', rank=rank, world_size=world)
        import sdf_amd
        from sdf_amd import dist, engine
        ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
        eng = engine.get_engine(0)
        dev = torch.device('cuda', 0)
        out = []
        for name, samples in (('ex_example', 2 ** 22), ('ex_weave', 2 ** 21), ('ex_blobby', 2 ** 24)):
            f = fixtures.build(name, ns)
            X, Y, Z, _ = core.grid_axes(tuple(map(tuple, BOUNDS[name])), samples=samples)
            m = eng.generate(f, X, Y, Z)
            want, wst = m.points(), m.stats()
            m.close()
            for chunks in (1, 1, 2):              # (the second call runs on the capacities the first one learned)
                soup, st = dist.generate_sharded_device(eng, f, X, Y, Z, 32, True, device=dev, chunks=chunks)
                got = soup.cpu().numpy().reshape(-1, 3)
                assert 'native' in st['exchange'] and st['world'] == world and st['chunks'] == chunks
                assert st['triangles'] == len(want) // 3 == sum(st['per_rank_triangles'])
                assert np.array_equal(got, want), (name, chunks)
                assert (st['skipped'], st['empty'], st['nonempty'], st['n_eval_voxels']) == (wst['skipped'], wst['empty'], wst['nonempty'], wst['n_eval_voxels'])
                out.append((name, chunks, st['n_retries'], st['per_rank_triangles']))
            # two steps in flight on the two lanes, collected in order
            a = dist.submit_sharded(eng, f, X, Y, Z, 32, True, device=dev, lane=0)
            b = dist.submit_sharded(eng, f, X, Y, Z, 32, True, device=dev, lane=1)
            for step in (a, b):
                soup, st = dist.collect_sharded(step)
                assert np.array_equal(soup.cpu().numpy().reshape(-1, 3), want)
        dist.shutdown_native()
        td.destroy_process_group()
        q.put((rank, 'ok', out))
    except BaseException:
        import traceback
        q.put((rank, 'ERROR', traceback.format_exc()))
        raise


@pytest.mark.parametrize('world,skip_shard,first_cap', [(2, False, 0), (3, True, 0), (2, True, 700)],
                         ids=['2-ranks', '3-ranks-sharded-skip', '2-ranks-sharded-skip-tiny-first-capacity'])
def test_native_exchange_between_processes_on_one_device(world, skip_shard, first_cap, tmp_path):
    """The library's OWN multi-GPU step (csrc/sdf_comm.hip: sdf_generate_sharded_async / sdf_exchange_wait -- shards of
    the work list, skip test shared out and its verdicts gathered, slabs, expansion, capacity hints, the retry every
    rank takes on the same gathered headers, two lanes) between several real processes.  RCCL refuses two ranks on one
    GPU, so the five RCCL entry points the library dlopens are provided by tests/native/mock_rccl.cpp (shared-memory
    all-gather, SDF_RCCL_LIB), and torch (gloo) only carries the communicator ids (SDF_DIST_NATIVE=force).  Every rank
    must end with the single-GPU soup, bit for bit, for example / weave (two-pass, 4-slot libm kernel) / blobby, with one
    and two shards per rank, and the ranks must agree on retries and per-rank counts."""
    import shutil
    import subprocess
    import torch.multiprocessing as mp
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    mock = str(tmp_path / 'mock_rccl.so')
    subprocess.run([hipcc, '-shared', '-fPIC', '-O2', '-o', mock, os.path.join(ROOT, 'tests', 'native', 'mock_rccl.cpp')],
                   check=True, capture_output=True, timeout=300)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 11 * world + (5 if skip_shard else 0) + (3 if first_cap else 0)
    procs = [ctx.Process(target=_native_exchange_worker, args=(r, world, port, q, mock, skip_shard, first_cap)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = [q.get(timeout=600) for _ in procs]
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.terminate()
    errors = [o for o in out if o[1] == 'ERROR']
    assert not errors, 'rank %d failed:\n%s' % (errors[0][0], errors[0][2])
    assert all(o[2] == out[0][2] for o in out)                       # same retries, same per-rank counts on every rank
    if first_cap:
        assert any(r[2] >= 1 for r in out[0][2])                     # the tiny first capacity was flagged and repeated
    else:
        assert all(r[2] == 0 for r in out[0][2])


def test_core_module_seams_are_the_batch_loop(ns, eng):
    """`core._skip`, `core._worker`, `core._marching_cubes` (reference sdf/core.py:16-18, 28-43, 45-60): the module-level
    functions a reference user can call on ONE job return what `generate` computes for that batch -- the skip verdict, None /
    [] / the batch's slice of the soup bit for bit -- and the marching-cubes seam returns skimage's soup and raises like it"""
    f = fixtures.build('ex_example', ns)
    X, Y, Z, _ = core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=2 ** 18)
    mesh = eng.generate(f, X, Y, Z, 32, True)
    pts, offs, kinds = mesh.points(), mesh.batch_offsets(), mesh.kinds()
    mesh.close()
    b = seen = 0
    for xs in range(0, len(X), 32):
        for ys in range(0, len(Y), 32):
            for zs in range(0, len(Z), 32):
                job = (X[xs:xs + 33], Y[ys:ys + 33], Z[zs:zs + 33])
                assert core._skip(f, job) == (kinds[b] == 0)
                r = core._worker(f, job, None, True)
                if kinds[b] == 0:
                    assert r is None
                elif kinds[b] == 1:
                    assert len(r) == 0
                else:
                    assert np.array_equal(r, pts[3 * offs[b]:3 * offs[b + 1]])
                    seen += 1
                assert core._worker(f, job, None, False) is not None       # sparse=False never skips
                b += 1
    assert b == len(kinds) and seen >= 8
    name = 'gyroid33'
    got = core._marching_cubes(MC['vol_' + name])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), MC['soup_' + name].view(np.uint32))
    with pytest.raises(RuntimeError):
        core._marching_cubes(np.full((4, 4, 4), 0.0, np.float32))            # no surface
    with pytest.raises(ValueError):
        core._marching_cubes(MC['vol_all_positive'])                         # level outside the volume's range
    with pytest.raises(ValueError):
        core._marching_cubes(np.ones((4, 4)))


# ---- `generate` for a host caller: 16-byte records over PCIe, the float64 soup made on host threads (sdf_generate_records) ----
REC_CASES = [('ex_example', 'gen_example_s17'), ('ex_example', 'gen_example_s22'), ('ex_blobby', 'gen_blobby_s20'), ('ex_gearlike', 'gen_gearlike_s20'),
             ('ex_weave', 'gen_weave_s19'), ('ex_pawn', 'gen_pawn_s16'), ('ex_knurling', 'gen_knurling_s16')]


@pytest.mark.parametrize('name,gold', REC_CASES, ids=[g for _, g in REC_CASES])
def test_records_mode_gives_the_same_soup_and_serves_every_reader(name, gold, ns, eng):
    """the second call of a model on a grid takes the records path (the first leaves the capacity hint): the soup the host threads
    make is the device's float64 soup bit for bit, for 1, 3 and all workers; STL records, the weld, ranges, batch offsets and
    sdf_mesh_emit_device of such a mesh are those of an ordinary one"""
    import torch
    d = np.load(os.path.join(GOLDEN, gold + '.npz'))
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    m0 = eng.generate(f, X, Y, Z, 32, True)
    want, st0 = m0.points(), m0.stats()
    stl0, (wp0, wc0), off0 = m0.stl_records().copy(), m0.weld(), m0.batch_offsets()
    m0.close()
    if name not in TRIG:
        assert hashlib.sha256(want.tobytes()).digest() == d['sha256'].tobytes()
    for workers in (1, 3, 0):
        m = eng.generate(f, X, Y, Z, 32, True, records=True)
        got = m.points(workers)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        st = m.stats()
        assert all(st[k] == st0[k] for k in ('triangles', 'skipped', 'empty', 'nonempty', 'n_eval_voxels', 'n_ambiguous_cells')) and st['n_retries'] == 0
        if workers == 3:       # the readers that want the float64 soup on the device (k_expand on demand), before and after points()
            assert np.array_equal(m.batch_offsets(), off0)
            t = m.n_triangles
            assert np.array_equal(m.points_range(t // 3, t // 2 - t // 3), want[3 * (t // 3):3 * (t // 2)])
            assert m.stl_records().tobytes() == stl0.tobytes()
            wp, wc = m.weld()
            assert np.array_equal(wp, wp0) and np.array_equal(wc, wc0)
            buf = torch.zeros(9 * t, dtype=torch.float64, device='cuda:0')
            m.emit_device(buf.data_ptr())
            assert np.array_equal(buf.cpu().numpy().reshape(-1, 3), want)
            assert np.array_equal(m.points(2), want)               # (now a plain copy of the expanded soup)
        m.close()
    m = eng.generate(f, X, Y, Z, 32, True, records=True)           # a reader first, points() never
    assert m.stl_records().tobytes() == stl0.tobytes()
    m.close()


def test_records_mode_slab_that_is_too_small_is_sized_again(ns, eng):
    """the capacity hint is keyed by model and grid SHAPE: the same shape over other bounds needs more triangles than the hint
    says -- the slab overflows on the device, is sized from the count and the call repeated"""
    f = fixtures.build('ex_example', ns)
    n = 97
    far = np.linspace(0.55, 1.6, n)            # a corner of the model: few triangles
    A = np.linspace(-1.1, 1.1, n)
    m = eng.generate(f, far, far, far, 32, True); few = m.n_triangles; m.close()
    m = eng.generate(f, A, A, A, 32, True); want = m.points(); m.close()
    assert 0 < few < len(want) // 3 // 4
    m = eng.generate(f, far, far, far, 32, True); m.close()          # (the hint of this shape says `few` again)
    m = eng.generate(f, A, A, A, 32, True, records=True)
    assert m.stats()['n_retries'] >= 1 and np.array_equal(m.points(), want)
    m.close()
    m = eng.generate(f, A, A, A, 32, True, records=True)             # ... and the next call fits at once
    assert m.stats()['n_retries'] == 0 and np.array_equal(m.points(5), want)
    m.close()


def test_generate_drop_in_returns_the_reference_soup_through_records(ns):
    """f.generate() on fresh model objects: the second call finds the first one's hint (keyed by the tape's CONTENT) and goes through
    the records; both return the reference's points"""
    d = np.load(os.path.join(GOLDEN, 'gen_example_s22.npz'))
    for workers in (1, 4, 8):
        f = fixtures.build('ex_example', ns)
        pts = f.generate(samples=2 ** 22, workers=workers, verbose=False)
        assert hashlib.sha256(pts.tobytes()).digest() == d['sha256'].tobytes()
    # a model with centre vertices (Lewiner's tilings with a vertex inside the cell: the slab's raw area)
    d = np.load(os.path.join(GOLDEN, 'gen_blobby_s20.npz'))
    for _ in range(2):
        f = fixtures.build('ex_blobby', ns)
        pts = f.generate(samples=2 ** 20, verbose=False)
        assert hashlib.sha256(pts.tobytes()).digest() == d['sha256'].tobytes()


# ---- every register file of k_mesh: sdf_mesh_inst.hip is built for the plain and the trig family, each with six register files
# (saved-point, saved-distance slots) and two schemes (one pass / k_mesh + k_scan_items + k_emit2).  The models of
# fixtures.SLOT_FIXTURES reach the files the value fixtures do not (tests/test_register_slots.py checks which file each one
# lowers to); here each is meshed under both schemes and compared with the tree-walking checker. ----

SLOTS = sorted(fixtures.SLOT_FIXTURES)
BOUNDS_SLOTS = np.load(os.path.join(GOLDEN, 'bounds_slots.npz'))
VALUES_SLOTS = np.load(os.path.join(GOLDEN, 'values_slots.npz'))
_SLOT_ORACLE = {}          # (model, batch size, sparse) -> the checker's generate, shared by the two schemes


def _slot_grid(name):
    """about 2^20 samples over the reference's bounds; no axis is a multiple of either batch size (32, 13): the last batch on
    every axis is ragged"""
    lo, hi = BOUNDS_SLOTS[name]
    return tuple(np.linspace(lo[i], hi[i], n) for i, n in enumerate((103, 97, 105)))


@pytest.mark.parametrize('scheme', [0, 1], ids=['one_pass', 'two_pass'])
@pytest.mark.parametrize('name', SLOTS)
def test_register_files_and_schemes_match_the_checker(name, scheme, ns, oracle_lib, eng):
    f = fixtures.build(name, ns)
    trig = is_trig(tape.lower(f))
    X, Y, Z = _slot_grid(name)
    extent = max(X[-1] - X[0], Y[-1] - Y[0], Z[-1] - Z[0])
    eng.set_twopass(scheme)
    try:
        soups = {}
        for bs in (32, 13):
            for sparse in (True, False):
                key = (name, bs, sparse)
                o = _SLOT_ORACLE.pop(key, None) if scheme else _SLOT_ORACLE.get(key)
                if o is None:
                    o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
                    if not scheme:
                        _SLOT_ORACLE[key] = o
                m = eng.generate(f, X, Y, Z, bs, sparse)
                pts, kinds, st, offs = m.points(), m.kinds(), m.stats(), m.batch_offsets()
                m.close()
                where = (name, scheme, bs, sparse)
                assert np.array_equal(kinds, o.kinds), where
                assert (st['skipped'], st['empty'], st['nonempty']) == tuple(int((o.kinds == k).sum()) for k in (0, 1, 2)), where
                assert st['n_eval_voxels'] == o.n_eval and st['triangles'] == len(o.points) // 3, where
                assert offs[0] == 0 and offs[-1] == len(o.points) // 3 and np.array_equal(np.diff(offs) > 0, o.kinds == 2), where
                assert pts.shape == o.points.shape, where
                if trig:
                    assert np.abs(pts - o.points).max() <= 1e-5 * extent, where       # north-star tolerance
                    assert (pts == o.points).mean() > 0.999, where
                else:
                    assert np.array_equal(pts, o.points), where
                soups[bs, sparse] = pts
        assert (o.kinds == 2).sum() >= 100                  # (the last one: batch size 13, dense)
        # the interval passes (prepass at this file's LDS size, culling at its interval state) change no bit
        (p1, k1, s1), (p0, k0, s0) = _both_ways(eng, f, X, Y, Z)
        assert s0['n_pruned_instrs'] == 0 and s0['n_sampled_voxels'] == s0['n_eval_voxels']
        assert np.array_equal(k1, k0) and np.array_equal(p1, p0) and np.array_equal(p1, soups[32, True])
    finally:
        eng.set_twopass(-1)
    if scheme == 0:                # the records path (16-byte records, the soup made on host threads): once per model
        m = eng.generate(f, X, Y, Z, 32, True, records=True)
        got = m.points()
        m.close()
        assert got.shape == soups[32, True].shape and np.array_equal(got.view(np.uint64), soups[32, True].view(np.uint64))
    # f(P) on the device (the evaluation kernels, not k_mesh) against the checker and the reference
    P = VALUES_SLOTS['P']
    v, o, ref = eng.eval_points(f, P), oracle_lib.evaluate(f, P), VALUES_SLOTS['v_' + name]
    assert np.array_equal(np.isnan(v), np.isnan(o))
    ok = ~np.isnan(o)
    if trig:
        assert np.all(np.abs(v[ok] - o[ok]) <= value_tolerance(o[ok], P[ok]))
    else:
        assert np.array_equal(v, o, equal_nan=True)
    ok = ~np.isnan(ref)
    assert np.all(np.abs(v[ok] - ref[ok]) <= value_tolerance(ref[ok], P[ok]))


FORCED = ['ex_example', 'ex_gearlike', 'ex_pawn', 'slots_plain_4_2']
# every count of sdf_stats but the capacity retries (a fresh context has no size hint yet); the times are not compared
_COUNTS = [k for k, _ in SdfStats._fields_ if k.startswith('n_') and k != 'n_retries'] + ['mesh_kernel']


@pytest.mark.parametrize('name', FORCED)
def test_forced_register_file_gives_the_same_soup(name, ns, eng, monkeypatch):
    """SDF_MESH_SLOTS (read when a context is created) forces any register file that holds the tape: which one meshes is a
    register-allocation choice and must not change a bit -- soup, classification, batch offsets and every count, under both
    schemes, are the session engine's (which takes the smallest file)"""
    from sdf_amd import engine
    f = fixtures.build(name, ns)
    t = tape.lower(f)
    files = files_holding(t)
    assert len(files) >= 3, (name, files)
    bounds = BOUNDS[name] if name in BOUNDS.files else BOUNDS_SLOTS[name]
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, bounds)), samples=2 ** 18)
    m = eng.generate(f, X, Y, Z, 32, True)
    want = (m.points(), m.kinds(), m.batch_offsets(), m.stats())
    m.close()
    assert want[3]['nonempty'] > 0
    for k in files:
        monkeypatch.setenv('SDF_MESH_SLOTS', str(k))
        for scheme in (0, 1):
            e = engine.Engine(0)
            dt = engine.DeviceTape(e, t)
            try:
                e.set_twopass(scheme)
                m = e.generate(dt, X, Y, Z, 32, True)
                got = (m.points(), m.kinds(), m.batch_offsets(), m.stats())
                m.close()
            finally:
                dt._fin(); e._fin()
            where = (name, k, scheme)
            assert got[0].shape == want[0].shape and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), where
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), where
            assert [got[3][c] for c in _COUNTS] == [want[3][c] for c in _COUNTS], where


def test_device_tape_refuses_a_ninth_slot(ns, oracle_lib, eng):
    """validate_tape (csrc/sdf_ctx.hip) refuses a tape that declares more slots than the (8,8) register file holds; one that
    declares exactly 8 + 8 is accepted and meshed by that file"""
    from sdf_amd import engine
    f = ns['sphere'](1) & ns['box'](1.5)
    t = tape.lower(f)
    for n_p, n_d in ((9, 1), (1, 9), (9, 9)):
        with pytest.raises(engine.SdfHipError, match='more register slots'):
            engine.DeviceTape(eng, tape.Tape(t.code, t.consts, n_p, n_d, 3))
    dt = engine.DeviceTape(eng, tape.Tape(t.code, t.consts, 8, 8, 3))
    X, Y, Z, _ = core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=2 ** 18)
    o = oracle_lib.generate(f, X, Y, Z, 32, True)
    try:
        for scheme in (0, 1):
            eng.set_twopass(scheme)
            m = eng.generate(dt, X, Y, Z, 32, True)
            pts, kinds = m.points(), m.kinds()
            m.close()
            assert np.array_equal(kinds, o.kinds) and np.array_equal(pts, o.points), scheme
    finally:
        eng.set_twopass(-1)
        dt._fin()
