"""The allocation hook (sdf_test_fail_alloc) walked through the feature calls whose device blocks go through the library's hooked
allocator (csrc/sdf_runtime.h: the scratch block of sdf_render_host, sdf_distance_texture_host and sdf_mesh_level_set_host, the three
blocks of sdf_mesh_weld): every failing call returns 1 with the allocator's message, the free device memory is what it was, and the
first call that gets through returns what the un-hooked call returned.  The shapes make every scratch block at least 16 MiB, so that
a leaked one shows in hipMemGetInfo.  The hook injects a HOST-side allocation error: nothing on the device faults."""
import ctypes

import numpy as np
import pytest

from sdf_amd import engine
from sdf_amd.render import camera
from test_export_gpu import Soup, random_soup
from test_level_set_gpu import icosphere

pytestmark = pytest.mark.gpu


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def _recorded(monkeypatch, lib, name):
    """the return codes of the entry point `name` from now on"""
    real, seen = getattr(lib, name), []

    def entry(*args):
        seen.append(real(*args))
        return seen[-1]
    monkeypatch.setattr(lib, name, entry)
    return seen


def _walk(eng, call, rcs, most=4):
    """call() un-hooked (which also warms it), then with the n-th allocation failing for n = 1, 2, ... until it succeeds; returns
    (the un-hooked result, the first hooked result that succeeded, the number of failures)"""
    lib = eng.lib
    want = call()
    eng.synchronize()
    f0 = _free(lib)
    failures, got = 0, None
    try:
        for n in range(1, most + 2):
            del rcs[:]
            lib.sdf_test_fail_alloc(n)
            try:
                got = call()
            except engine.SdfHipError as e:
                lib.sdf_test_fail_alloc(0)
                failures += 1
                assert rcs == [1] and 'emory' in str(e) and b'emory' in lib.sdf_last_error(), (rcs, e)
                assert _free(lib) == f0, (n, f0, _free(lib))
                continue
            lib.sdf_test_fail_alloc(0)
            assert rcs == [0], rcs
            break
    finally:
        lib.sdf_test_fail_alloc(0)
    assert got is not None and 1 <= failures <= most, failures
    assert _free(lib) == f0                                     # the scratch block is freed before the call returns
    return want, got, failures


def test_render_scratch_goes_through_the_hook(ns, eng, monkeypatch):
    """render_buffers of sphere(1) at 1024 x 512: 37 B per pixel, 19 MB of scratch"""
    f = eng.tape_for(ns['sphere'](1))                            # (lowered and uploaded once: the walk is through the call alone)
    w, h = 1024, 512
    frame, t_near, t_far, _ = camera(((-1, -1, -1), (1, 1, 1)), w, h)
    rcs = _recorded(monkeypatch, eng.lib, 'sdf_render_host')
    want, got, _ = _walk(eng, lambda: eng.render_buffers(f, frame, w, h, t_near=t_near, t_far=t_far), rcs)
    assert want['status'].any() and not want['status'].all()
    for k in ('depth', 'normal', 'steps', 'status'):
        assert np.array_equal(got[k], want[k]), k


def test_distance_texture_scratch_goes_through_the_hook(eng, monkeypatch):
    """distance_texture of a 1024 x 2048 mask with one filled disc: 13 B per pixel, 27 MB of scratch"""
    r, c = np.mgrid[0:1024, 0:2048]
    mask = (r - 500) ** 2 + (c - 900) ** 2 <= 300 ** 2
    rcs = _recorded(monkeypatch, eng.lib, 'sdf_distance_texture_host')
    want, got, _ = _walk(eng, lambda: eng.distance_texture(mask), rcs)
    assert want[500, 900] == -np.sqrt(90001.0) and want[500, 1201] == 1.0 and want[0, 0] > 0
    assert np.array_equal(got, want)


def test_level_set_scratch_goes_through_the_hook(eng, monkeypatch):
    """level_set of the icosphere: voxel size 2 / 119 and half width 3 make the work grid 128^3, 12 B per voxel, 25 MB of scratch"""
    P, T = icosphere(3)
    rcs = _recorded(monkeypatch, eng.lib, 'sdf_mesh_level_set_host')
    want, got, _ = _walk(eng, lambda: eng.mesh_level_set(P, T, 2.0 / 119, 3), rcs)
    assert want[1].size > 100000 and (want[1] < 0).any() and (want[1] > 0).any()
    assert np.array_equal(got[0], want[0]) and got[1].shape == want[1].shape and np.array_equal(got[1], want[1])


def test_weld_blocks_go_through_the_hook(eng):
    """sdf_mesh_weld on 400,000 random triangles (1.2 M rows: 9.6 MB per key block, 28.8 MB of unique rows): a failure at any of its
    three blocks -- the two results, taken after the sort, among them -- frees what was taken and leaves the mesh unwelded, so that
    the next sdf_mesh_weld welds it"""
    lib = eng.lib
    n_tris = 400000
    warm = Soup(eng, random_soup(3))
    try:
        warm.mesh.weld()
    finally:
        warm.close()
    first = Soup(eng, random_soup(n_tris))                      # the un-hooked result
    try:
        want = tuple(a.copy() for a in first.mesh.weld())
    finally:
        first.close()
    assert len(want[0]) == 3 * n_tris
    s = Soup(eng, random_soup(n_tris))
    try:
        eng.synchronize()
        f0 = _free(lib)
        nu = ctypes.c_int64(0)
        pts, cells = np.empty((3 * n_tris, 3), np.float64), np.empty((n_tris, 3), np.int64)
        f64p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
        failures, rc = 0, -1
        for n in range(1, 12):
            lib.sdf_test_fail_alloc(n)
            rc = lib.sdf_mesh_weld(s.mesh.handle, ctypes.byref(nu))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error(), (rc, lib.sdf_last_error())
            assert _free(lib) == f0, (n, f0, _free(lib))
            assert lib.sdf_mesh_weld_fetch(s.mesh.handle, pts.ctypes.data_as(f64p), cells.ctypes.data_as(i64p)) == 1   # no weld was left behind
            assert b'call sdf_mesh_weld first' in lib.sdf_last_error()
        assert rc == 0 and failures == 3 and nu.value == 3 * n_tris, (rc, failures, nu.value)
        held = f0 - _free(lib)                                  # the mesh owns the unique rows and the index now (32 B per row), and nothing else
        assert 96 * n_tris <= held <= 96 * n_tris + (8 << 20), (held, 96 * n_tris)
        got = s.mesh.weld()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
    eng.synchronize()
    assert _free(lib) >= f0
