"""Host binding of the HIP library (sdf_amd/csrc -> libsdf_hip.so) through its C ABI
(include/sdf_hip.h).  ctypes only: no torch types cross the boundary; torch is used by
sdf_amd/dist.py for the RCCL exchange, not here.

There is NO CPU fallback: if the shared library is missing, or no MI355X is visible,
every entry point raises.  (The CPU checker under oracle/ is test infrastructure and is
never imported from this package.)
"""
import ctypes
import os
import threading
import weakref

import numpy as np

from . import tape as _tape

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SDF_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libsdf_hip.so')   # (SDF_HIP_LIB: another build of the library, for A/B timing)

PRECISION_F64 = 0
PRECISION_F32 = 1

_c_i64 = ctypes.c_int64
_vp = ctypes.c_void_p
_f64p = ctypes.POINTER(ctypes.c_double)
_f32p = ctypes.POINTER(ctypes.c_float)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


class SdfExchangeStats(ctypes.Structure):
    """mirror of `sdf_exchange_stats` in include/sdf_hip.h"""
    _fields_ = [(k, ctypes.c_int64) for k in ('n_batches', 'n_skipped', 'n_empty', 'n_nonempty', 'n_triangles', 'n_grid_voxels',
                                               'n_eval_voxels', 'n_ambiguous_cells', 'n_sampled_voxels', 'n_pruned_instrs',
                                               'n_retries', 'chunks', 'world', 'slab_bytes')] + \
               [(k, ctypes.c_double) for k in ('ms_mesh', 'ms_exchange', 'ms_expand', 'ms_total')] + \
               [('per_rank_triangles', ctypes.c_int64 * 64)]


class SdfMoments(ctypes.Structure):
    """mirror of `sdf_moments` in include/sdf_hip.h"""
    _fields_ = [('sums', ctypes.c_double * 11), ('origin', ctypes.c_double * 3), ('box_lo', ctypes.c_double * 3),
                ('box_hi', ctypes.c_double * 3), ('n_triangles', _c_i64), ('n_zero_area', _c_i64), ('n_nonfinite', _c_i64)]


CENSUS_FIELDS = ('vertices', 'faces', 'collapsed', 'edges', 'paired', 'boundary', 'misoriented', 'nonmanifold', 'euler', 'closed',
                 'oriented')


class SdfEdgeCensus(ctypes.Structure):
    """mirror of `sdf_edge_census` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in CENSUS_FIELDS]


class SdfComponents(ctypes.Structure):
    """mirror of `sdf_components` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in ('n_shells', 'n_vertices', 'n_triangles', 'rounds')] + \
               [(k, ctypes.c_double) for k in ('ms_label', 'ms_number')]


SIMPLIFY_FIELDS = ('clusters', 'triangles_in', 'triangles_out', 'collapsed', 'mean_fallback', 'flat')


class SdfSimplifyStats(ctypes.Structure):
    """mirror of `sdf_simplify_stats` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in SIMPLIFY_FIELDS] + [('kernel_ms', ctypes.c_double)]


ADAPTIVE_FIELDS = ('triangles_in', 'triangles_out', 'collapsed', 'levels', 'mean_fallback', 'flat')
ADAPTIVE_MAX_LEVELS = 10


class SdfAdaptiveStats(ctypes.Structure):
    """mirror of `sdf_adaptive_stats` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in ADAPTIVE_FIELDS] + [('clusters_used', _c_i64 * (ADAPTIVE_MAX_LEVELS + 1)),
                                                         ('vertices', _c_i64 * (ADAPTIVE_MAX_LEVELS + 1)), ('kernel_ms', ctypes.c_double)]


MEND_FIELDS = ('triangles_in', 'triangles_out', 'collapsed', 'duplicates', 'cancelled', 'faces')


class SdfMendStats(ctypes.Structure):
    """mirror of `sdf_mend_stats` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in MEND_FIELDS] + [('kernel_ms', ctypes.c_double)]


SNAP_FIELDS = ('vertices', 'left', 'snapped', 'held', 'flat', 'nan')


class SdfSnapStats(ctypes.Structure):
    """mirror of `sdf_snap_stats` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in SNAP_FIELDS] + [('kernel_ms', ctypes.c_double)]


CONTOUR_COUNTS = ('n_points', 'n_contours', 'n_segments', 'nonfinite_cells', 'rounds')


class SdfContourCounts(ctypes.Structure):
    """mirror of `sdf_contour_counts` in include/sdf_hip.h"""
    _fields_ = [(k, _c_i64) for k in CONTOUR_COUNTS]


class SdfStats(ctypes.Structure):
    """mirror of `sdf_stats` in include/sdf_hip.h"""
    _fields_ = [
        ('n_batches', _c_i64), ('n_skipped', _c_i64), ('n_empty', _c_i64), ('n_nonempty', _c_i64),
        ('n_triangles', _c_i64), ('n_grid_voxels', _c_i64), ('n_eval_voxels', _c_i64),
        ('n_ambiguous_cells', _c_i64), ('n_work_begin', _c_i64), ('n_work_end', _c_i64),
        ('n_retries', _c_i64),
        ('ms_prepass', ctypes.c_double), ('ms_mesh', ctypes.c_double), ('ms_emit', ctypes.c_double),
        ('ms_total', ctypes.c_double), ('n_pruned_instrs', _c_i64), ('n_batch_instrs', _c_i64),
        ('n_sampled_voxels', _c_i64), ('ms_mesh_device', ctypes.c_double), ('sclk_mhz', ctypes.c_double),
        ('t_mesh_first_us', ctypes.c_double), ('t_mesh_last_us', ctypes.c_double), ('mesh_kernel', ctypes.c_int64),
    ]


# name -> (restype, argtypes); this table is also what tests/test_host.py checks against the header
ABI = {
    'sdf_abi_version': (ctypes.c_int, []),
    'sdf_build_info': (ctypes.c_char_p, []),
    'sdf_last_error': (ctypes.c_char_p, []),
    'sdf_device_count': (ctypes.c_int, []),
    'sdf_device_mem_info': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    'sdf_test_fail_alloc': (ctypes.c_int, [ctypes.c_int]),
    'sdf_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    'sdf_ctx_destroy': (ctypes.c_int, [_vp]),
    'sdf_ctx_set_stream': (ctypes.c_int, [_vp, _vp]),
    'sdf_ctx_set_prune': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_set_cull': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_set_twopass': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_set_tail_order': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_set_defer': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_set_cull_levels': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_ctx_synchronize': (ctypes.c_int, [_vp]),
    'sdf_ctx_trim': (ctypes.c_int, [_vp]),
    'sdf_tape_create': (ctypes.c_int, [_vp, _u32p, ctypes.c_uint32, _f64p, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    'sdf_tape_set_prune_info': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16),
                                               ctypes.c_uint32]),
    'sdf_tape_set_intervals': (ctypes.c_int, [_vp, ctypes.c_int]),
    'sdf_tape_destroy': (ctypes.c_int, [_vp]),
    'sdf_eval_points': (ctypes.c_int, [_vp, _vp, _c_i64, ctypes.c_int, _vp, ctypes.c_int]),
    'sdf_eval_points_host': (ctypes.c_int, [_vp, _f64p, _c_i64, ctypes.c_int, _f64p, ctypes.c_int]),
    'sdf_eval_grid_host': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p,
                                          ctypes.c_int, _f64p, ctypes.c_int]),
    'sdf_estimate_bounds': (ctypes.c_int, [_vp, _f64p, ctypes.c_int]),
    'sdf_tape_extern_count': (ctypes.c_int, [_vp]),
    'sdf_eval_extern_points_host': (ctypes.c_int, [_vp, _f64p, _c_i64, ctypes.c_int, _f64p, ctypes.c_int]),
    'sdf_eval_points_extern_host': (ctypes.c_int, [_vp, _f64p, _c_i64, ctypes.c_int, _f64p, _f64p, ctypes.c_int]),
    'sdf_generate_field': (ctypes.c_int, [_vp, _vp, _vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.POINTER(_vp)]),
    'sdf_marching_cubes': (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                          _c_i64, ctypes.POINTER(_c_i64)]),
    'sdf_marching_cubes_host': (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               _f32p, _c_i64, ctypes.POINTER(_c_i64)]),
    'sdf_mesh_level_set_host': (ctypes.c_int, [_vp, _f64p, _c_i64, ctypes.POINTER(ctypes.c_int32), _c_i64, ctypes.c_double,
                                               ctypes.c_int, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _f32p, _c_i64]),
    'sdf_distance_texture_host': (ctypes.c_int, [_vp, _u8p, _c_i64, _c_i64, _f64p]),
    'sdf_render_host': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_int, _f64p, _f64p,
                                       ctypes.POINTER(ctypes.c_int32), _u8p]),
    'sdf_render_last_kernel_ms': (ctypes.c_double, []),
    'sdf_generate': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int,
                                    ctypes.POINTER(_vp)]),
    'sdf_generate_to_device': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, _vp, _c_i64,
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_vp)]),
    'sdf_generate_to_device_async': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                    ctypes.c_int, _vp, ctypes.c_int64, ctypes.POINTER(_vp)]),
    'sdf_mesh_wait': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    'sdf_generate_records': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    'sdf_slab_bytes': (ctypes.c_size_t, [_c_i64, _c_i64]),
    'sdf_generate_compact_async': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, _vp, _c_i64,
                                                  _c_i64, ctypes.POINTER(_vp)]),
    'sdf_expand_slabs': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, _c_i64, _c_i64, _vp, _c_i64]),
    'sdf_comm_available': (ctypes.c_int, []),
    'sdf_comm_unique_id': (ctypes.c_int, [_vp]),
    'sdf_comm_create': (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    'sdf_comm_destroy': (ctypes.c_int, [_vp]),
    'sdf_generate_sharded_async': (ctypes.c_int, [_vp, _vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.POINTER(_vp)]),
    'sdf_exchange_wait': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_c_i64)]),
    'sdf_exchange_stats_get': (ctypes.c_int, [_vp, ctypes.POINTER(SdfExchangeStats)]),
    'sdf_exchange_destroy': (ctypes.c_int, [_vp]),
    'sdf_skip_kinds': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_int, _c_i64,
                                      _c_i64, ctypes.c_int, _vp]),
    'sdf_generate_from_kinds': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_int,
                                               _c_i64, _c_i64, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    'sdf_memcpy_to_host': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    'sdf_mesh_stats': (ctypes.c_int, [_vp, ctypes.POINTER(SdfStats)]),
    'sdf_mesh_triangles': (_c_i64, [_vp]),
    'sdf_mesh_emit_device': (ctypes.c_int, [_vp, _vp]),
    'sdf_mesh_emit_host': (ctypes.c_int, [_vp, _f64p]),
    'sdf_mesh_emit_host_workers': (ctypes.c_int, [_vp, _f64p, ctypes.c_int]),
    'sdf_mesh_emit_host_range': (ctypes.c_int, [_vp, _c_i64, _c_i64, _f64p]),
    'sdf_mesh_batch_offsets': (ctypes.c_int, [_vp, ctypes.POINTER(_c_i64)]),
    'sdf_mesh_emit_stl_host': (ctypes.c_int, [_vp, _vp]),
    'sdf_mesh_adopt_soup': (ctypes.c_int, [_vp, _vp, _c_i64, ctypes.POINTER(_vp)]),
    'sdf_mesh_weld': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    'sdf_mesh_weld_fetch': (ctypes.c_int, [_vp, _f64p, ctypes.POINTER(ctypes.c_int64)]),
    'sdf_mesh_vertex_normals': (ctypes.c_int, [_vp, _vp, ctypes.c_double, _f64p, ctypes.POINTER(ctypes.c_int64)]),
    'sdf_mesh_normals_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_vertex_thickness': (ctypes.c_int, [_vp, _vp, _f64p, ctypes.c_int, ctypes.c_int, _f64p, _u8p, ctypes.POINTER(ctypes.c_int32)]),
    'sdf_mesh_thickness_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_vertex_curvature': (ctypes.c_int, [_vp, _vp, ctypes.c_double, _f64p, _u8p, ctypes.POINTER(ctypes.c_int64)]),
    'sdf_mesh_curvature_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_triangle_deviation': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _f64p, ctypes.POINTER(ctypes.c_int32), _f64p]),
    'sdf_mesh_deviation_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_snap': (ctypes.c_int, [_vp, _vp, _f64p, ctypes.c_int, ctypes.POINTER(_vp), _f64p, _u8p, _f64p, ctypes.POINTER(ctypes.c_int32),
                                     ctypes.POINTER(SdfSnapStats)]),
    'sdf_mesh_emit_ply_host': (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    'sdf_mesh_moments': (ctypes.c_int, [_vp, _f64p, ctypes.POINTER(SdfMoments)]),
    'sdf_mesh_edge_census': (ctypes.c_int, [_vp, ctypes.POINTER(SdfEdgeCensus)]),
    'sdf_mesh_measure_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_components': (ctypes.c_int, [_vp, ctypes.POINTER(SdfComponents)]),
    'sdf_mesh_components_fetch': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _f64p]),
    'sdf_mesh_select_shells': (ctypes.c_int, [_vp, _u8p, _c_i64, ctypes.POINTER(_vp)]),
    'sdf_mesh_components_last_kernel_ms': (ctypes.c_double, []),
    'sdf_mesh_simplify': (ctypes.c_int, [_vp, _f64p, _f64p, ctypes.c_double, ctypes.POINTER(_vp), ctypes.POINTER(SdfSimplifyStats)]),
    'sdf_mesh_simplify_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_mesh_simplify_adaptive': (ctypes.c_int, [_vp, _f64p, _f64p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(_vp),
                                                  ctypes.POINTER(SdfAdaptiveStats)]),
    'sdf_mesh_simplify_adaptive_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_mesh_mend': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(SdfMendStats)]),
    'sdf_mesh_mend_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_contour_grid_host': (ctypes.c_int, [_vp, _f64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f64p, _f64p, ctypes.c_double,
                                             ctypes.POINTER(_vp), ctypes.POINTER(SdfContourCounts)]),
    'sdf_contour_host': (ctypes.c_int, [_vp, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_double,
                                        _f64p, ctypes.POINTER(_vp), ctypes.POINTER(SdfContourCounts)]),
    'sdf_contours_fetch': (ctypes.c_int, [_vp, _f64p, ctypes.POINTER(_c_i64), _u8p, ctypes.POINTER(ctypes.c_int32), _f64p]),
    'sdf_contours_destroy': (ctypes.c_int, [_vp]),
    'sdf_contour_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_mesh_overhangs': (ctypes.c_int, [_vp, _f64p, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_size_t, _f64p,
                                          ctypes.POINTER(_c_i64)]),
    'sdf_mesh_overhang_classes': (ctypes.c_int, [_vp, _f64p, ctypes.c_double, ctypes.c_double, _u8p]),
    'sdf_overhang_last_kernel_ms': (ctypes.c_double, [ctypes.POINTER(_c_i64)]),
    'sdf_mesh_support_rays': (ctypes.c_int, [_vp, _vp, _f64p, _c_i64, _f64p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp), _f64p,
                                             ctypes.POINTER(_c_i64)]),
    'sdf_support_rays_fetch': (ctypes.c_int, [_vp, _c_i64, ctypes.POINTER(ctypes.c_int32), _f64p, _u8p, ctypes.POINTER(ctypes.c_int32), _f64p]),
    'sdf_support_rays_destroy': (ctypes.c_int, [_vp]),
    'sdf_mesh_supports_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_generate_dual': (ctypes.c_int, [_vp, _vp, _f64p, ctypes.c_int, _f64p, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_c_i64), ctypes.POINTER(_vp)]),
    'sdf_dual_parts_fetch': (ctypes.c_int, [_vp, _f64p, _f64p, _f64p, ctypes.POINTER(_c_i64)]),
    'sdf_dual_parts_destroy': (ctypes.c_int, [_vp]),
    'sdf_generate_dual_last_kernel_ms': (ctypes.c_double, [_f64p]),
    'sdf_host_alloc': (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(_vp)]),
    'sdf_host_free': (ctypes.c_int, [_vp]),
    'sdf_mesh_kinds': (ctypes.c_int, [_vp, _u8p]),
    'sdf_mesh_prune_masks': (ctypes.c_int, [_vp, _u32p]),
    'sdf_mesh_destroy': (ctypes.c_int, [_vp]),
}
ABI_VERSION = 17


def build_info():
    """the toolchain that built the loaded library (csrc/build.sh records it: sdf_build_info)"""
    return load_library().sdf_build_info().decode()


def _strip_c_comments(text):
    """C / C++ source without its comments; string and character literals are left alone (a `//` inside a format string or
    a URL is not a comment)"""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch in '"\'':                                  # a literal: copy to its closing quote, honouring escapes
            j = i + 1
            while j < n and text[j] != ch:
                j += 2 if text[j] == '\\' else 1
            out.append(text[i:j + 1]); i = j + 1
        elif text.startswith('//', i):
            j = text.find('\n', i)
            i = n if j < 0 else j
        elif text.startswith('/*', i):
            j = text.find('*/', i + 2)
            i = n if j < 0 else j + 2
        else:
            out.append(ch); i += 1
    return ''.join(out)


def source_id():
    """sha256 (16 hex digits) over the library's sources -- sdf_amd/csrc/*.{h,hip,inc,sh,units} and the public header
    include/sdf_hip.h -- WITHOUT their comments and blank lines: what a committed rocprofv3 summary was taken on
    (tools/summarize_prof.py writes it, bench.py only quotes a summary whose id is this build's).  Editing a comment does
    not make a profile stale; editing code, a string literal or the exchange's host code does."""
    import glob
    import hashlib
    import re
    h = hashlib.sha256()
    here = os.path.dirname(os.path.abspath(__file__))
    d = os.path.join(here, 'csrc')
    files = sorted(glob.glob(os.path.join(d, '*'))) + [os.path.join(os.path.dirname(here), 'include', 'sdf_hip.h')]
    for f in files:
        ext = f.rsplit('.', 1)[-1]
        if os.path.isfile(f) and ext in ('h', 'hip', 'inc', 'sh', 'units'):
            text = open(f, encoding='utf-8', errors='replace').read()
            if ext in ('sh', 'units'):
                text = re.sub(r'(?m)^\s*#(?!!).*$', '', text)
            else:
                text = _strip_c_comments(text)
            text = '\n'.join(ln.rstrip() for ln in text.split('\n') if ln.strip())
            h.update(os.path.basename(f).encode()); h.update(text.encode())
    return h.hexdigest()[:16]

_lib = None
_lib_lock = threading.Lock()


class SdfHipError(RuntimeError):
    pass


# `sdf_field_fn` of include/sdf_hip.h
FIELD_FN = ctypes.CFUNCTYPE(ctypes.c_int, _vp, _f64p, _c_i64, _f64p)


def call_closure(fn, P):
    """a user closure on (N, d) points -> (N,) float64: the contract of a function decorated with the
    reference's @sdf3 / @op3 (reference README.md:258-295: returns (N,) or (N, 1))"""
    v = np.asarray(fn(P), dtype=np.float64).reshape(-1)
    if v.shape[0] != len(P):
        raise ValueError('a user SDF returned %d values for %d points' % (v.shape[0], len(P)))
    return v


def load_library(path=None):
    """dlopen libsdf_hip.so and attach the prototypes; raises if it was not built"""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise SdfHipError(
                '%s is missing: build the HIP extension first '
                '(python -c "import __graft_entry__ as g; g.build()"); sdf_amd has no CPU path' % p)
        lib = ctypes.CDLL(p)
        for name, (rt, at) in ABI.items():
            fn = getattr(lib, name)
            fn.restype = rt
            fn.argtypes = at
        if lib.sdf_abi_version() != ABI_VERSION:
            raise SdfHipError('libsdf_hip.so ABI %d != binding %d' % (lib.sdf_abi_version(), ABI_VERSION))
        if path is None:
            _lib = lib
        return lib


_REFUSED = 2          # an entry point's return value for arguments it refused before anything was allocated or launched (include/sdf_hip.h)


def _check(lib, rc):
    """nothing for 0; ValueError for a refusal (every `return 2` of csrc is an argument check); SdfHipError for any other failure --
    both with the text of sdf_last_error"""
    if rc != 0:
        msg = lib.sdf_last_error()
        raise (ValueError if rc == _REFUSED else SdfHipError)(msg.decode() if msg else 'sdf_hip error %d' % rc)


def _dp(a, t):
    return a.ctypes.data_as(t)


def _stats_dict(st, fields, **more):
    """the statistics dict of a ctypes struct: its integer `fields`, what the caller adds, kernel_ms"""
    return dict({k: int(getattr(st, k)) for k in fields}, **more, kernel_ms=float(st.kernel_ms))


def evaluator(eng, tape):
    """the field of `tape` as a host evaluator P -> (N,) float64: what a probe's definition on the host takes"""
    return lambda P: eng.eval_points(tape, P)


class DeviceTape:
    """a lowered model resident on the device (`sdf_tape*`)"""

    def __init__(self, eng, tape):
        self.engine = eng
        self.tape = tape
        self.handle = _vp()
        lib = eng.lib
        _check(lib, lib.sdf_tape_create(eng.ctx, _dp(tape.code, _u32p), len(tape.code),
                                        _dp(tape.consts, _f64p), len(tape.consts),
                                        tape.n_pslots, tape.n_dslots, ctypes.byref(self.handle)))
        self._fin = weakref.finalize(self, lib.sdf_tape_destroy, self.handle)
        if tape.rstart is not None and len(tape.rstart) == tape.n_instr:
            u16p = ctypes.POINTER(ctypes.c_uint16)
            _check(lib, lib.sdf_tape_set_prune_info(self.handle, _dp(tape.rstart, u16p), _dp(tape.lstart, u16p),
                                                    tape.n_instr))
        if not getattr(tape, 'intervals', True):      # (a model that is NaN everywhere, sdf_amd/tape.py: no interval pass at all)
            _check(lib, lib.sdf_tape_set_intervals(self.handle, 0))


class _PinnedBlock:
    """a block of the library's pinned host memory (sdf_host_alloc) that an ndarray can sit on: the
    array keeps this object as its base, and the block goes back to the library's free list when the
    last view of it is gone"""

    def __init__(self, lib, nbytes):
        p = _vp()
        _check(lib, lib.sdf_host_alloc(max(int(nbytes), 1), ctypes.byref(p)))
        self.ptr = p.value
        self.nbytes = int(nbytes)
        self._fin = weakref.finalize(self, lib.sdf_host_free, _vp(self.ptr))

    @property
    def __array_interface__(self):
        return {'shape': (self.nbytes,), 'typestr': '|u1', 'data': (self.ptr, False), 'version': 3}


def pinned_empty(lib, shape, dtype):
    """np.empty in pinned host memory (results of large device-to-host copies land here: PCIe rate
    instead of the ~10 GB/s of fresh pageable memory); falls back to np.empty when pinning fails"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    if n < (1 << 20):
        return np.empty(shape, dtype)
    try:
        blk = _PinnedBlock(lib, n)
    except SdfHipError:
        return np.empty(shape, dtype)
    return np.asarray(blk)[:n].view(dtype).reshape(shape)


class Mesh:
    """result of one `generate` call (`sdf_mesh*`): triangle soup resident on the device"""

    def __init__(self, eng, handle):
        self.engine = eng
        self.handle = handle
        self._fin = weakref.finalize(self, eng.lib.sdf_mesh_destroy, handle)

    @property
    def n_triangles(self):
        return int(self.engine.lib.sdf_mesh_triangles(self.handle))

    def wait(self):
        """collect a call submitted with generate(wait=False); returns `emitted`"""
        e = ctypes.c_int(0)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_wait(self.handle, ctypes.byref(e)))
        self.emitted = bool(e.value)
        return self.emitted

    def stats(self):
        st = SdfStats()
        _check(self.engine.lib, self.engine.lib.sdf_mesh_stats(self.handle, ctypes.byref(st)))
        d = {k: getattr(st, k) for k, _ in SdfStats._fields_}
        d.update(skipped=st.n_skipped, empty=st.n_empty, nonempty=st.n_nonempty,
                 batches=st.n_batches, triangles=st.n_triangles)
        return d

    def kinds(self):
        """per-batch classification in reference batch order: 0 skipped / 1 empty / 2 nonempty
        (3 = outside this rank's shard)"""
        n = self.stats()['n_batches']
        out = np.empty(max(n, 1), np.uint8)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_kinds(self.handle, _dp(out, _u8p)))
        return out[:n]

    def prune_masks(self):
        """(n_batches, 16) uint32: the interval prepass's skip / forced bits per batch (batch order,
        like kinds(); only the batches that were meshed used them)"""
        n = self.stats()['n_batches']
        out = np.zeros((max(n, 1), 16), np.uint32)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_prune_masks(self.handle, _dp(out, _u32p)))
        return out[:n]

    def points(self, workers=0):
        """(3T, 3) float64 world-space soup in reference order, on the host.  A mesh of `generate(records=True)`
        sends its 16-byte records and `workers` host threads (0: the machine's, at most 32; at most 64) make the soup
        from them (`sdf_mesh_emit_host_workers`); any other mesh copies its float64 soup"""
        t = self.n_triangles
        out = pinned_empty(self.engine.lib, (3 * t, 3), np.float64)
        if t:
            _check(self.engine.lib, self.engine.lib.sdf_mesh_emit_host_workers(self.handle, _dp(out, _f64p), int(workers or 0)))
        return out

    def points_range(self, first_tri, n_tris):
        """rows of triangles [first_tri, first_tri + n_tris) of the soup: (3 * n_tris, 3) float64"""
        out = pinned_empty(self.engine.lib, (3 * int(n_tris), 3), np.float64)
        if n_tris:
            _check(self.engine.lib, self.engine.lib.sdf_mesh_emit_host_range(self.handle, int(first_tri), int(n_tris),
                                                                             _dp(out, _f64p)))
        return out

    def batch_offsets(self):
        """(n_batches + 1,) int64: where each batch's triangles start in this shard's soup (reference
        batch order; equal neighbours = the batch contributed nothing)"""
        n = self.stats()['n_batches']
        out = np.zeros(n + 1, np.int64)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_batch_offsets(self.handle, _dp(out, ctypes.POINTER(_c_i64))))
        return out

    def emit_device(self, device_ptr):
        """write the (3T,3) float64 soup into caller-owned device memory (e.g. a torch tensor)"""
        _check(self.engine.lib, self.engine.lib.sdf_mesh_emit_device(self.handle, _vp(device_ptr)))

    def weld(self):
        """(unique points (U, 3) float64 in lexicographic order, cells (T, 3) int64): what
        `np.unique(points, axis=0, return_inverse=True)` gives the reference's `_mesh`
        (reference sdf/core.py:160-164), sorted and deduplicated on the device"""
        nu = ctypes.c_int64(0)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_weld(self.handle, ctypes.byref(nu)))
        pts = pinned_empty(self.engine.lib, (nu.value, 3), np.float64)
        cells = pinned_empty(self.engine.lib, (self.n_triangles, 3), np.int64)
        if nu.value:
            _check(self.engine.lib, self.engine.lib.sdf_mesh_weld_fetch(self.handle, _dp(pts, _f64p),
                                                                       _dp(cells, ctypes.POINTER(ctypes.c_int64))))
        return pts, cells

    def _derived(self, handle, **attrs):
        """the Mesh that select, simplify, simplify_adaptive, mend or snap made, from its handle: nothing emitted, and the
        attributes its maker names"""
        m = Mesh(self.engine, handle)
        m.emitted = False
        vars(m).update(attrs)
        return m

    def _welded(self):
        """number of unique vertices; welds (on the device) if that has not happened yet"""
        nu = ctypes.c_int64(0)
        _check(self.engine.lib, self.engine.lib.sdf_mesh_weld(self.handle, ctypes.byref(nu)))
        return int(nu.value)

    def vertex_normals(self, sdf_or_tape, eps):
        """(normals (U, 3) float64, n_flat): the normalised central difference of the FIELD, step eps, at the U welded vertices
        (sdf_mesh_vertex_normals, csrc/sdf_normals.hip; defined by tests/normals_ref.py and reproduced bit
        for bit).  A vertex where the difference is zero or NaN is flat: its normal is (0, 0, 0) and it is counted in n_flat.
        The normals also stay on the device with the mesh, for `ply_records(normals=True)`.  A model with user closures takes
        the same definition over `Engine.eval_points` on the host (and keeps nothing on the device).  Raises ValueError,
        before any device work, for an eps that is not finite and positive and for an engine in float32 precision."""
        eng = self.engine
        eps = float(eps)
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError('eps must be finite and positive, got %r' % eps)
        dt, ev = eng._probe_tape(sdf_or_tape, 'vertex_normals takes the gradient')
        if ev:
            from . import meshfile
            return meshfile.vertex_normals(ev, self.weld()[0], eps)
        nu = self._welded()
        out = pinned_empty(eng.lib, (nu, 3), np.float64)
        flat = ctypes.c_int64(0)
        _check(eng.lib, eng.lib.sdf_mesh_vertex_normals(self.handle, dt.handle, eps, _dp(out, _f64p), ctypes.byref(flat)))
        return out, int(flat.value)

    def vertex_thickness(self, sdf_or_tape, normal_eps, start, min_step, t_far, step_scale=1.0, max_steps=256, refine=16):
        """(thickness (U,) float64, status (U,) uint8, steps (U,) int32): the wall's ray thickness at the U welded vertices
        (sdf_mesh_vertex_thickness, csrc/sdf_thickness.hip; defined by tests/thickness_ref.py and reproduced
        bit for bit).  From every vertex a ray is sphere-traced inward, along the negated field normal (step normal_eps), from
        t = start through the solid until the field is positive again, advancing by max(-value * step_scale, min_step), and the
        crossing is bisected `refine` times.  status: 0 OPEN (beyond t_far or out of max_steps: +inf), 1 THICK, 2 THIN (outside
        already at `start`: the thickness is `start`, an upper bound), 3 FLAT (no gradient: NaN), 4 NAN (the field was NaN on the
        ray: NaN).  A model with user closures takes the same definition over `Engine.eval_points` on the host.  Raises ValueError,
        before any device work, for the parameters the C entry refuses and for an engine in float32 precision."""
        from .thickness import check_params, vertex_thickness      # (the package's attribute `thickness` is the function)
        eng = self.engine
        params = check_params(normal_eps, start, min_step, t_far, step_scale, max_steps, refine)
        dt, ev = eng._probe_tape(sdf_or_tape, 'vertex_thickness marches')
        if ev:
            return vertex_thickness(ev, self.weld()[0], *params)
        nu = self._welded()
        th, status, steps = np.empty(nu, np.float64), np.empty(nu, np.uint8), np.empty(nu, np.int32)
        p6 = np.array(params[:5] + [0.0], np.float64)
        _check(eng.lib, eng.lib.sdf_mesh_vertex_thickness(self.handle, dt.handle, _dp(p6, _f64p), params[5], params[6], _dp(th, _f64p),
                                                          _dp(status, _u8p), _dp(steps, ctypes.POINTER(ctypes.c_int32))))
        return th, status, steps

    def vertex_curvature(self, sdf_or_tape, eps):
        """(curv (U, 4) float64: mean, gauss, k1, k2; status (U,) uint8; counts (3,) int64): the curvature of the FIELD's level set at
        the U welded vertices (sdf_mesh_vertex_curvature, csrc/sdf_curvature.hip; defined by
        tests/curvature_ref.py and reproduced bit for bit).  The gradient and the Hessian are second differences of 19 values at
        step eps; mean and Gaussian curvature are closed forms in them, k1 >= k2 the principal curvatures; convex is positive.
        status: 0 CURVED, 1 FLAT (no gradient), 2 NAN (the field or a result was not finite); a vertex that is not CURVED holds
        np.nan's bits in all four.  counts: the vertices of each status, counted on the device.  A model with user closures takes
        the same definition over `Engine.eval_points` on the host.  Raises ValueError, before any device work, for an eps that is
        not finite and positive and for an engine in float32 precision."""
        from .curvature import check_params, vertex_curvature       # (the package's attribute `curvature` is the function)
        eng = self.engine
        eps = check_params(eps)
        dt, ev = eng._probe_tape(sdf_or_tape, 'vertex_curvature takes second differences')
        if ev:
            curv, status = vertex_curvature(ev, self.weld()[0], eps)
            return curv, status, np.bincount(status, minlength=3).astype(np.int64)
        nu = self._welded()
        curv, status, counts = np.empty((nu, 4), np.float64), np.empty(nu, np.uint8), np.zeros(3, np.int64)
        _check(eng.lib, eng.lib.sdf_mesh_vertex_curvature(self.handle, dt.handle, eps, _dp(curv, _f64p), _dp(status, _u8p),
                                                          _dp(counts, ctypes.POINTER(ctypes.c_int64))))
        return curv, status, counts

    def triangle_deviation(self, sdf_or_tape, order=2):
        """(dev (T,) float64, at (T,) int32, sumsq (T,) float64): how far every triangle of the soup lies from the zero set of the
        field (sdf_mesh_triangle_deviation, csrc/sdf_deviation.hip; defined by tests/deviation_ref.py and
        reproduced bit for bit).  The field is sampled at the (order+1)(order+2)/2 points of a barycentric lattice (order 1 .. 8;
        sample 0 is the first corner): dev is the sampled value of largest magnitude (NaN once a sample is NaN), at the index of that
        sample, sumsq the sum of the squared values.  It is one-sided, mesh to surface, and |f| is a distance only where the field is
        one.  Needs no weld.  A model with user closures takes the same definition over `Engine.eval_points` on the host.  Raises
        ValueError, before any device work, for an order outside 1 .. 8 and for an engine in float32 precision."""
        from .deviation import check_order, triangle_deviation
        eng = self.engine
        order = check_order(order)
        dt, ev = eng._probe_tape(sdf_or_tape, 'triangle_deviation samples')
        if ev:
            return triangle_deviation(ev, np.asarray(self.points()).reshape(-1, 3, 3), order)
        t = self.n_triangles
        dev, at, sumsq = np.empty(t, np.float64), np.empty(t, np.int32), np.empty(t, np.float64)
        _check(eng.lib, eng.lib.sdf_mesh_triangle_deviation(self.handle, dt.handle, order, _dp(dev, _f64p), _dp(at, ctypes.POINTER(ctypes.c_int32)),
                                                            _dp(sumsq, _f64p)))
        return dev, at, sumsq

    def snap(self, sdf_or_tape, eps, tol, max_move, iters=4):
        """a new Mesh: this one with its welded vertices put back on the zero set of the field (sdf_mesh_snap, csrc/sdf_deviation.hip;
        DESIGN.md section 4q; defined by tests/deviation_ref.py and reproduced bit for bit).  Up to `iters` Newton steps
        q - f(q) g / |g|^2 with g the central difference of step eps; a vertex stops as SNAPPED (1) once |f(q)| <= tol, as HELD (2)
        where a step would take it farther than max_move from where it began, as FLAT (3) where the field has no gradient, as NAN
        (4, back where it began) where the field is NaN, and is LEFT (0) when the steps run out.  The result owns its soup -- the
        moved points through the welded cells, in triangle order and winding -- and serves every reader; it carries `snap_stats`
        (vertices, left, snapped, held, flat, nan, kernel_ms), `snap_result` = (points (U, 3), status (U,) uint8, residual (U,)) in
        THIS mesh's weld order and `snap_evals` (U,) int32.  Vertices that land on one point make collapsed triangles (`mend`
        drops them); creases are not restored and topology is not preserved.  This mesh stays valid.  A model with user closures
        takes the same definition over `Engine.eval_points` on the host, and the new soup is uploaded.  Raises ValueError, before
        any device work, for the parameters the C entry refuses and for an engine in float32 precision."""
        from .deviation import STATUS_NAMES, check_snap, vertex_snap
        eng = self.engine
        eps, tol, max_move, iters = check_snap(eps, tol, max_move, iters)
        dt, ev = eng._probe_tape(sdf_or_tape, 'snap steps')
        if ev:
            from . import core
            pts, cells = self.weld()
            q, status, residual, evals = vertex_snap(ev, pts, eps, tol, max_move, iters)
            held = core.adopted(q[cells])                          # (the upload lives as long as the mesh over it)
            m = held.__enter__()
            m._adopted, m.emitted = held, False
            stats = dict({'vertices': len(pts)}, kernel_ms=0.0, **{n.lower(): int((status == c).sum()) for c, n in enumerate(STATUS_NAMES)})
        else:
            nu = self._welded()
            q, status = np.empty((nu, 3), np.float64), np.empty(nu, np.uint8)
            residual, evals = np.empty(nu, np.float64), np.empty(nu, np.int32)
            p4 = np.array([eps, tol, max_move, 0.0], np.float64)
            h, st = _vp(), SdfSnapStats()
            _check(eng.lib, eng.lib.sdf_mesh_snap(self.handle, dt.handle, _dp(p4, _f64p), iters, ctypes.byref(h), _dp(q, _f64p), _dp(status, _u8p),
                                                  _dp(residual, _f64p), _dp(evals, ctypes.POINTER(ctypes.c_int32)), ctypes.byref(st)))
            m, stats = self._derived(h), _stats_dict(st, SNAP_FIELDS)
        m.snap_stats, m.snap_result, m.snap_evals = stats, (q, status, residual), evals
        return m

    def ply_records(self, normals=False):
        """(vertex_bytes, face_bytes) uint8: the body of a binary little-endian PLY file of the welded mesh, packed on the device
        (sdf_mesh_emit_ply_host): U records of float32 x, y, z (12 bytes; with normals=True + float32 nx, ny, nz: 24 bytes --
        needs `vertex_normals` first) and T records of uint8 3 + 3 x int32 (13 bytes)"""
        eng = self.engine
        nu, t = self._welded(), self.n_triangles
        vb = pinned_empty(eng.lib, (nu * (24 if normals else 12),), np.uint8)
        fb = pinned_empty(eng.lib, (13 * t,), np.uint8)
        if nu == 0 or t == 0:
            return vb, fb
        _check(eng.lib, eng.lib.sdf_mesh_emit_ply_host(self.handle, 1 if normals else 0, vb.ctypes.data_as(_vp), fb.ctypes.data_as(_vp)))
        return vb, fb

    def moments(self, origin=None):
        """the raw moments of the soup, summed on the device (sdf_mesh_moments, csrc/sdf_measure.hip; defined
        by tests/measure_ref.py and reproduced bit for bit): a dict of `sums` (11 float64: sum |n|, sum det, 3 first-moment and 6
        second-moment totals about `origin`), `origin` (3,), `box` (2, 3) and the counts `triangles`, `zero_area`, `nonfinite`.
        origin=None takes the midpoint of the bounding box.  `measure.derive` turns the totals into volume, area, centroid and
        inertia.  Needs no weld."""
        eng = self.engine
        o = None
        if origin is not None:
            o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
            if o.shape != (3,):
                raise ValueError('origin must have 3 components, got %r' % (origin,))
        out = SdfMoments()
        _check(eng.lib, eng.lib.sdf_mesh_moments(self.handle, _dp(o, _f64p) if o is not None else None, ctypes.byref(out)))
        return {'sums': np.array(out.sums[:], np.float64), 'origin': np.array(out.origin[:], np.float64),
                'box': np.array([out.box_lo[:], out.box_hi[:]], np.float64), 'triangles': int(out.n_triangles),
                'zero_area': int(out.n_zero_area), 'nonfinite': int(out.n_nonfinite)}

    def edge_census(self):
        """the edge census of the welded mesh, counted on the device (sdf_mesh_edge_census; welds first if that has not happened):
        a dict of the integers `vertices`, `faces`, `collapsed`, `edges`, `paired`, `boundary`, `misoriented`, `nonmanifold`,
        `euler` and the booleans `closed`, `oriented` (tests/measure_ref.py defines them)"""
        eng = self.engine
        self._welded()
        out = SdfEdgeCensus()
        _check(eng.lib, eng.lib.sdf_mesh_edge_census(self.handle, ctypes.byref(out)))
        d = {k: int(getattr(out, k)) for k in CENSUS_FIELDS}
        d['closed'], d['oriented'] = bool(d['closed']), bool(d['oriented'])
        return d

    def _labelled(self):
        """the `sdf_components` of this mesh; labels (and welds) on the device if that has not happened yet"""
        eng = self.engine
        out = SdfComponents()
        _check(eng.lib, eng.lib.sdf_mesh_components(self.handle, ctypes.byref(out)))
        return out

    def components(self):
        """the connected shells of the welded mesh, labelled on the device (sdf_mesh_components, csrc/sdf_components.hip; DESIGN.md
        section 4h; defined by tests/components_ref.py and reproduced exactly): a dict of `count` K, `rounds` (the passes the
        labelling took, the verifying one included), `vertex_shell` (U,) int32, `triangle_shell` (T,) int32 and per shell
        `triangles` (K,) int64, `vertices` (K,) int64, `bounds` (K, 2, 3) float64.  Shells are numbered by their lexicographically
        smallest vertex.  The arrays stay on the device with the mesh: a second call only copies them."""
        eng = self.engine
        c = self._labelled()
        k, i32p, i64p = int(c.n_shells), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_c_i64)
        out = {'count': k, 'rounds': int(c.rounds),
               'vertex_shell': pinned_empty(eng.lib, (int(c.n_vertices),), np.int32),
               'triangle_shell': pinned_empty(eng.lib, (int(c.n_triangles),), np.int32),
               'triangles': np.empty(k, np.int64), 'vertices': np.empty(k, np.int64), 'bounds': np.empty((k, 2, 3), np.float64)}
        if k:
            _check(eng.lib, eng.lib.sdf_mesh_components_fetch(self.handle, _dp(out['vertex_shell'], i32p), _dp(out['triangle_shell'], i32p),
                                                              _dp(out['triangles'], i64p), _dp(out['vertices'], i64p), _dp(out['bounds'], _f64p)))
        return out

    def shell_summary(self):
        """`components()` without the per-vertex and per-triangle arrays: `count`, `rounds`, `triangles`, `vertices`, `bounds` --
        all that choosing shells by size needs to bring over the link"""
        eng = self.engine
        c = self._labelled()
        k, i64p = int(c.n_shells), ctypes.POINTER(_c_i64)
        out = {'count': k, 'rounds': int(c.rounds), 'triangles': np.empty(k, np.int64), 'vertices': np.empty(k, np.int64),
               'bounds': np.empty((k, 2, 3), np.float64)}
        if k:
            _check(eng.lib, eng.lib.sdf_mesh_components_fetch(self.handle, None, None, _dp(out['triangles'], i64p),
                                                              _dp(out['vertices'], i64p), _dp(out['bounds'], _f64p)))
        return out

    def select(self, keep_mask):
        """a new Mesh of the triangles whose shell is kept (keep_mask: K booleans, one per shell of `components()`), in soup order,
        bit for bit, compacted on the device (sdf_mesh_select_shells).  The selection owns its soup and serves every reader --
        points, stl_records, weld, ply_records, vertex_normals, moments, edge_census, components; this mesh stays valid.  A mask
        of another length raises ValueError before any launch; an all-False mask gives a mesh of 0 triangles."""
        eng = self.engine
        mask = np.ascontiguousarray(np.asarray(keep_mask).reshape(-1) != 0, dtype=np.uint8)
        self._labelled()
        h = _vp()
        _check(eng.lib, eng.lib.sdf_mesh_select_shells(self.handle, _dp(mask, _u8p), len(mask), ctypes.byref(h)))
        return self._derived(h)

    def simplify(self, origin, cell, reg=1e-3):
        """a new Mesh: this one simplified on the device (sdf_mesh_simplify, csrc/sdf_simplify.hip; defined by
        tests/simplify_ref.py and reproduced bit for bit).  The welded vertices are clustered on the uniform grid (origin (3,), cell
        (3,) > 0), every cluster gets one representative placed by its quadric (regularised by reg towards the mean of its vertices,
        kept inside its cell), and the triangles whose three clusters differ survive, in order and winding.  Duplicates and
        oppositely wound pairs are not removed unless the result is mended (`mend`; `edge_census` reports them).  The result owns its soup and serves every reader;
        its `simplify_stats` is a dict of clusters, triangles_in, triangles_out, collapsed, mean_fallback, flat and kernel_ms.
        This mesh stays valid.  ValueError, before any device work, for a cell that is not positive and finite, an origin that
        is not finite or a negative reg; SdfHipError for a vertex that is not finite or a cell too small for the key."""
        eng = self.engine
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        c = np.ascontiguousarray(cell, dtype=np.float64).reshape(-1)
        if o.shape != (3,) or c.shape != (3,):
            raise ValueError('simplify: origin and cell have 3 components each, got %r and %r' % (origin, cell))
        h, st = _vp(), SdfSimplifyStats()
        _check(eng.lib, eng.lib.sdf_mesh_simplify(self.handle, _dp(o, _f64p), _dp(c, _f64p), float(reg), ctypes.byref(h), ctypes.byref(st)))
        return self._derived(h, simplify_stats=_stats_dict(st, SIMPLIFY_FIELDS))

    def simplify_adaptive(self, origin, cell, tolerance, levels=5, reg=1e-3):
        """a new Mesh: this one simplified to a tolerance on the device (sdf_mesh_simplify_adaptive, csrc/sdf_simplify.hip; DESIGN.md
        section 4p; defined by tests/adaptive_ref.py and reproduced bit for bit).  Level L = 0 .. levels is the clustering of
        `simplify` on the grid (origin, cell x 2^L); a cluster is accepted when the squared-area-weighted mean squared distance of
        its representative from the planes of the triangles that touch it is at most tolerance^2 (model units; not a Hausdorff
        bound), level 0 always; every welded vertex takes the coarsest accepted cluster it falls into, and the triangles whose
        three clusters differ survive, in order and winding.  Flat faces collapse to a few triangles, creases and fillets stay
        fine.  levels=0 is `simplify(origin, cell)`, tolerance=inf is `simplify(origin, cell * 2 ** levels)`.  The result owns its
        soup and serves every reader; its `simplify_stats` is a dict of triangles_in, triangles_out, collapsed, levels, the lists
        clusters_used and vertices (one entry per level), mean_fallback, flat, kernel_ms and tolerance.  This mesh stays valid.
        ValueError, before any device work, for what `simplify` refuses, a tolerance that is negative, NaN or no real number, levels
        that is no integer from 0 to 10 or a cell x 2^levels that is not finite; SdfHipError for a vertex that is not finite or a
        cell too small for the key."""
        from .simplify import check_levels, check_tolerance
        eng = self.engine
        tol = check_tolerance(tolerance, 'tolerance')
        lv = check_levels(levels, 'levels')
        if tol is None:
            raise ValueError('simplify_adaptive: tolerance must be a real number >= 0 (inf is allowed), got None')
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        c = np.ascontiguousarray(cell, dtype=np.float64).reshape(-1)
        if o.shape != (3,) or c.shape != (3,):
            raise ValueError('simplify_adaptive: origin and cell have 3 components each, got %r and %r' % (origin, cell))
        h, st = _vp(), SdfAdaptiveStats()
        _check(eng.lib, eng.lib.sdf_mesh_simplify_adaptive(self.handle, _dp(o, _f64p), _dp(c, _f64p), float(reg), tol, lv, ctypes.byref(h),
                                                           ctypes.byref(st)))
        stats = _stats_dict(st, ADAPTIVE_FIELDS, clusters_used=[int(n) for n in st.clusters_used[:lv + 1]], vertices=[int(n) for n in st.vertices[:lv + 1]])
        return self._derived(h, simplify_stats=dict(stats, tolerance=tol))

    def mend(self):
        """a new Mesh: this one mended on the device (sdf_mesh_mend, csrc/sdf_mend.hip; defined by
        tests/mend_ref.py and reproduced exactly).  Of the welded cells, those with two equal indices are dropped; of the cells of
        one face (the same three vertices), as many on either winding cancel, and otherwise the first in soup order of the majority
        winding survives alone.  Survivors keep their order, their winding and the bits of their nine doubles.  Nothing is
        re-oriented, and a wall that collapsed only in part keeps a non-manifold rim (`edge_census` reports it).  The result owns
        its soup and serves every reader; its `mend_stats` is a dict of triangles_in, triangles_out, collapsed, duplicates,
        cancelled, faces and kernel_ms.  This mesh stays valid.  ValueError for a mesh that has been closed (its handle is gone)."""
        eng = self.engine
        if not self._fin.alive:
            raise ValueError('mend: this mesh has been closed')
        h, st = _vp(), SdfMendStats()
        _check(eng.lib, eng.lib.sdf_mesh_mend(self.handle, ctypes.byref(h), ctypes.byref(st)))
        return self._derived(h, mend_stats=_stats_dict(st, MEND_FIELDS))

    def overhangs(self, directions, sin_limit, bed_tol, max_scratch_bytes=0):
        """build directions rated on the device (sdf_mesh_overhangs, csrc/sdf_overhang.hip; defined by
        tests/overhang_ref.py::rate and reproduced bit for bit): for UNIT directions (K, 3), a dict of `lo`, `hi` (K,) -- the
        extremes of the soup along each direction --, `sums` (K, 3) -- twice the overhanging area, six times the support prisms'
        volume, twice the area on the bed -- and the counts `overhang_triangles`, `contact_triangles` (K,) int64.
        `overhang.derive` turns the totals into areas, volume and height.  max_scratch_bytes: the cap of the chunk partials of a
        slab of directions (0: 64 MiB); no bit depends on it.  Needs no weld.  ValueError, before any device work, for what the C
        entry refuses: no direction, a direction not of unit length to 1e-12, sin_limit outside [0, 1), a negative bed_tol."""
        eng = self.engine
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError('directions must have the shape (K, 3), got %r' % (d.shape,))
        k = len(d)
        values, counts = np.empty((max(k, 1), 5), np.float64), np.empty((max(k, 1), 2), np.int64)
        _check(eng.lib, eng.lib.sdf_mesh_overhangs(self.handle, _dp(d, _f64p), k, float(sin_limit), float(bed_tol), int(max_scratch_bytes),
                                                   _dp(values, _f64p), _dp(counts, ctypes.POINTER(_c_i64))))
        return {'lo': values[:, 0].copy(), 'hi': values[:, 1].copy(), 'sums': values[:, 2:5].copy(),
                'overhang_triangles': counts[:, 0].copy(), 'contact_triangles': counts[:, 1].copy()}

    def overhang_classes(self, direction, sin_limit, bed_tol):
        """(T,) uint8, the class of every triangle for ONE unit direction, by the predicates of `overhangs`
        (sdf_mesh_overhang_classes): 0 neither, 1 overhang, 2 bed contact, 3 non-finite"""
        eng = self.engine
        d = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1)
        if d.shape != (3,):
            raise ValueError('direction must have 3 components, got %r' % (direction,))
        out = np.zeros(max(self.n_triangles, 1), np.uint8)
        _check(eng.lib, eng.lib.sdf_mesh_overhang_classes(self.handle, _dp(d, _f64p), float(sin_limit), float(bed_tol), _dp(out, _u8p)))
        return out[:self.n_triangles]

    def support_rays(self, sdf_or_tape, directions, sin_limit, bed_tol, start, min_step, step_scale=1.0, max_steps=256, refine=16):
        """support rays traced through the field of a model on the device (sdf_mesh_support_rays, csrc/sdf_supports.hip and
        csrc/sdf_overhang.hip; defined by tests/supports_ref.py::supports and reproduced bit for bit): for UNIT
        directions (K, 3), a dict of `lo`, `hi` (K,), `sums` (K, 5), `counts` (K, 5) int64 -- rays that ended BED, PART, BURIED,
        UNRESOLVED, NAN -- and `rays`, a list of K tuples (triangle (M,) int32, height (M,) float64, status (M,) uint8, steps (M,)
        int32, origin (M, 3) float64).  `supports.derive` turns the sums into volumes and areas.  Needs no weld.  A model with user
        closures takes the same definition over `Engine.eval_points` on the host.  ValueError, before any device work, for what the C
        entry refuses and for an engine in float32 precision."""
        from .supports import check_params, support_rays_host
        eng = self.engine
        d, params = check_params(directions, sin_limit, bed_tol, start, min_step, step_scale, max_steps, refine)
        dt, ev = eng._probe_tape(sdf_or_tape, 'support_rays marches')
        k = len(d)
        if ev:
            soup = self.points().reshape(-1, 3, 3)
            got = [support_rays_host(ev, soup, d[i], *params) for i in range(k)]
            return {'lo': np.array([g['lo'] for g in got]), 'hi': np.array([g['hi'] for g in got]),
                    'sums': np.array([g['sums'] for g in got]).reshape(k, 5), 'counts': np.array([g['counts'] for g in got], np.int64).reshape(k, 5),
                    'rays': [(g['triangle'], g['height'], g['status'], g['steps'], g['origin']) for g in got]}
        values, counts = np.empty((k, 7), np.float64), np.empty((k, 6), np.int64)
        p8 = np.array(params[:5] + [0.0, 0.0, 0.0], np.float64)
        h = _vp()
        i32p = ctypes.POINTER(ctypes.c_int32)
        _check(eng.lib, eng.lib.sdf_mesh_support_rays(self.handle, dt.handle, _dp(d, _f64p), k, _dp(p8, _f64p), params[5], params[6],
                                                      ctypes.byref(h), _dp(values, _f64p), _dp(counts, ctypes.POINTER(_c_i64))))
        try:
            rays = []
            for i in range(k):
                m = int(counts[i, 5])
                tri, height, status = np.empty(m, np.int32), np.empty(m, np.float64), np.empty(m, np.uint8)
                steps, origin = np.empty(m, np.int32), np.empty((m, 3), np.float64)
                if m:
                    _check(eng.lib, eng.lib.sdf_support_rays_fetch(h, i, _dp(tri, i32p), _dp(height, _f64p), _dp(status, _u8p), _dp(steps, i32p),
                                                                   _dp(origin, _f64p)))
                rays.append((tri, height, status, steps, origin))
        finally:
            eng.lib.sdf_support_rays_destroy(h)
        return {'lo': values[:, 0].copy(), 'hi': values[:, 1].copy(), 'sums': values[:, 2:7].copy(), 'counts': counts[:, :5].copy(), 'rays': rays}

    def stl_records(self):
        """T x 50-byte binary STL records (normals computed on the device)"""
        t = self.n_triangles
        out = pinned_empty(self.engine.lib, (50 * t,), np.uint8)
        if t:
            _check(self.engine.lib, self.engine.lib.sdf_mesh_emit_stl_host(self.handle, out.ctypes.data_as(_vp)))
        return out

    def close(self):
        self._fin()


COMM_ID_BYTES = 128          # SDF_COMM_ID_BYTES


class DeviceSoup:
    """a float64 soup in LIBRARY memory on the device (9 doubles per triangle): the result of an exchange step.  It
    exposes `__cuda_array_interface__` (zero-copy view for torch / cupy: `torch.as_tensor(soup, device=...)`) and can
    copy itself to the host.  Valid until the next step is submitted on the same lane of its communicator."""

    def __init__(self, eng, ptr, n_tris, keep=None):
        self.engine, self.ptr, self.n_triangles, self._keep = eng, int(ptr or 0), int(n_tris), keep

    @property
    def __cuda_array_interface__(self):
        return {'shape': (9 * self.n_triangles,), 'typestr': '<f8', 'data': (self.ptr, False), 'version': 2, 'strides': None}

    def to_host(self, first_tri=0, n_tris=None):
        """(3n, 3) float64 ndarray of triangles [first_tri, first_tri + n_tris)"""
        n = self.n_triangles - first_tri if n_tris is None else int(n_tris)
        out = pinned_empty(self.engine.lib, (3 * n, 3), np.float64)
        if n:
            _check(self.engine.lib, self.engine.lib.sdf_memcpy_to_host(self.engine.ctx, out.ctypes.data_as(_vp),
                                                                       _vp(self.ptr + 72 * int(first_tri)), 72 * n))
        return out


class Exchange:
    """one sharded step in flight (`sdf_exchange*`)"""

    def __init__(self, comm, handle, tape):
        self.comm, self.handle, self._tape = comm, handle, tape
        self._fin = weakref.finalize(self, comm.engine.lib.sdf_exchange_destroy, handle)
        comm._live.add(self)          # (a communicator that is closed first takes its steps with it: Comm.close)

    def wait(self):
        """the step's one host synchronisation -> (DeviceSoup, stats dict)"""
        lib = self.comm.engine.lib
        p, n = _vp(), _c_i64(0)
        _check(lib, lib.sdf_exchange_wait(self.handle, ctypes.byref(p), ctypes.byref(n)))
        st = SdfExchangeStats()
        _check(lib, lib.sdf_exchange_stats_get(self.handle, ctypes.byref(st)))
        d = {k: getattr(st, k) for k, _ in SdfExchangeStats._fields_ if k != 'per_rank_triangles'}
        d['per_rank_triangles'] = [int(v) for v in st.per_rank_triangles[:st.world]]
        d.update(batches=st.n_batches, skipped=st.n_skipped, empty=st.n_empty, nonempty=st.n_nonempty, triangles=st.n_triangles,
                 payload='16-byte triangle records (local coordinates) + per-batch transform', exchange='rccl (native)')
        return DeviceSoup(self.comm.engine, p.value, n.value, keep=self), d

    def close(self):
        self._fin()


class Comm:
    """the ranks of one multi-GPU job (`sdf_comm*`): RCCL communicators + persistent exchange buffers, 1 or 2 lanes.
    Creation is collective: every rank calls it with the ids rank 0 drew (`Comm.unique_ids`)."""

    @staticmethod
    def available(lib):
        """(True, '') if librccl loads in this process, else (False, why) -- local, nothing collective"""
        if lib.sdf_comm_available():
            return True, ''
        return False, (lib.sdf_last_error() or b'').decode(errors='replace')

    @staticmethod
    def unique_ids(lib, n_lanes=2):
        buf = ctypes.create_string_buffer(COMM_ID_BYTES * n_lanes)
        for l in range(n_lanes):
            _check(lib, lib.sdf_comm_unique_id(ctypes.cast(ctypes.byref(buf, COMM_ID_BYTES * l), _vp)))
        return buf.raw

    def __init__(self, eng, ids, rank, world):
        self.engine, self.rank, self.world = eng, int(rank), int(world)
        self.n_lanes = len(ids) // COMM_ID_BYTES
        self.handle = _vp()
        raw = ctypes.create_string_buffer(bytes(ids), len(ids))
        _check(eng.lib, eng.lib.sdf_comm_create(eng.ctx, ctypes.cast(raw, _vp), self.n_lanes, self.rank, self.world,
                                                ctypes.byref(self.handle)))
        self._fin = weakref.finalize(self, eng.lib.sdf_comm_destroy, self.handle)
        self._live = weakref.WeakSet()          # steps (Exchange) that still hold a handle into this communicator

    def submit(self, sdf, X, Y, Z, batch_size=32, sparse=True, chunks=1, lane=0):
        eng = self.engine
        dt = eng.tape_for(sdf)
        if dt.tape.externs:
            raise ValueError('a model with user closures is sharded through the host protocol (sdf_amd.dist with HostCodec)')
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        h = _vp()
        _check(eng.lib, eng.lib.sdf_generate_sharded_async(self.handle, dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y),
                                                           _dp(Z, _f64p), len(Z), int(batch_size), 1 if sparse else 0,
                                                           eng.precision, int(chunks), int(lane), ctypes.byref(h)))
        return Exchange(self, h, dt)

    def close(self):
        """destroy the communicator -- after the steps that point into it (an sdf_exchange handle must not outlive its
        sdf_comm: its destructor looks at the communicator's lanes)"""
        for x in list(self._live):
            x.close()
        self._fin()


class Engine:
    """one HIP context (`sdf_ctx*`) on one device"""

    def __init__(self, device=0):
        self.lib = load_library()
        n = self.lib.sdf_device_count()
        if n <= 0:
            raise SdfHipError('no HIP device visible (sdf_amd has no CPU path): %s'
                              % (self.lib.sdf_last_error() or b'').decode())
        self.device = device
        self.ctx = _vp()
        _check(self.lib, self.lib.sdf_ctx_create(device, ctypes.byref(self.ctx)))
        self._fin = weakref.finalize(self, self.lib.sdf_ctx_destroy, self.ctx)
        self.precision = PRECISION_F64
        self._tapes = weakref.WeakValueDictionary()

    def set_stream(self, stream_ptr):
        _check(self.lib, self.lib.sdf_ctx_set_stream(self.ctx, _vp(stream_ptr)))

    def set_prune(self, enabled):
        """interval prepass of generate on / off (default on; results are identical)"""
        _check(self.lib, self.lib.sdf_ctx_set_prune(self.ctx, int(bool(enabled))))

    def set_cull(self, enabled):
        """interval culling of cell groups inside a batch on / off (default on; results are identical)"""
        _check(self.lib, self.lib.sdf_ctx_set_cull(self.ctx, int(bool(enabled))))

    def set_tail_order(self, on):
        """hand the tail of the work list to the workgroups by descending cost (default) or in order; same results"""
        _check(self.lib, self.lib.sdf_ctx_set_tail_order(self.ctx, int(bool(on))))

    def set_defer(self, on):
        """one-kernel meshing: sparse tiles + deferred emission (default) or dense tiles + parking; same results"""
        _check(self.lib, self.lib.sdf_ctx_set_defer(self.ctx, int(bool(on))))

    def set_cull_levels(self, levels):
        """interval levels of the culling pass: 2, 3 or 0 = the library's choice by the tape (default); same results"""
        _check(self.lib, self.lib.sdf_ctx_set_cull_levels(self.ctx, int(levels)))

    def set_twopass(self, mode):
        """meshing scheme: 0 one kernel (look-back + parking), 1 three kernels (sample / number / emit), -1 the
        library's choice by the tape's length (default); results are identical"""
        _check(self.lib, self.lib.sdf_ctx_set_twopass(self.ctx, int(mode)))

    def synchronize(self):
        _check(self.lib, self.lib.sdf_ctx_synchronize(self.ctx))

    def trim(self):
        """return the library's cached device blocks to the driver (before a job of a very different size)"""
        _check(self.lib, self.lib.sdf_ctx_trim(self.ctx))

    # -- models --
    def tape_for(self, sdf):
        """lower `sdf` NOW (boolean smoothing constants are evaluation-time state in the
        reference, so nothing is cached across calls beyond identical tapes)"""
        if isinstance(sdf, DeviceTape):
            return sdf
        t = sdf if isinstance(sdf, _tape.Tape) else _tape.lower(sdf)
        key = (t.code.tobytes(), t.consts.tobytes(), tuple(id(fn) for fn, _ in t.externs))
        dt = self._tapes.get(key)
        if dt is None:
            dt = DeviceTape(self, t)
            self._tapes[key] = dt
        return dt

    def _probe_tape(self, sdf, verb):
        """the seven field probes, behind the checks of their own parameters: refuse float32 precision (`verb`: what the probe does
        in float64), then (the device tape, its `evaluator` if it reads user closures -- the probe's definition on the host serves
        those -- and None if not: the C call)"""
        if self.precision != PRECISION_F64:
            raise ValueError('%s in float64 only; this engine is set to float32 precision' % verb)
        dt = self.tape_for(sdf)
        return dt, evaluator(self, dt) if dt.tape.externs else None

    # -- f(P) --
    def eval_points(self, sdf, pts):
        dt = self.tape_for(sdf)
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] not in (2, 3):
            raise ValueError('points must be (N,2) or (N,3)')
        if dt.tape.externs:
            return self._eval_points_hybrid(dt, pts)
        out = np.empty(len(pts), np.float64)
        if len(pts):
            _check(self.lib, self.lib.sdf_eval_points_host(dt.handle, _dp(pts, _f64p), len(pts), pts.shape[1],
                                                           _dp(out, _f64p), self.precision))
        return out

    def _eval_points_hybrid(self, dt, pts):
        """f(P) of a model that contains user closures (`extern` leaves): the device runs the tape twice --
        first to find the point every closure is asked at (its argument after the transforms above it), then,
        with the closures' values (computed here, by the user's own NumPy code), for the result"""
        ext = dt.tape.externs
        n, dim = pts.shape
        if n == 0:
            return np.empty(0, np.float64)
        if dt.tape.n_instr == 2:          # the model IS one closure: nothing for the device to do
            return call_closure(ext[0][0], pts.copy())
        epts = np.empty((len(ext), n, 3), np.float64)
        _check(self.lib, self.lib.sdf_eval_extern_points_host(dt.handle, _dp(pts, _f64p), n, dim, _dp(epts, _f64p),
                                                              self.precision))
        vals = np.empty((len(ext), n), np.float64)
        for k, (fn, d) in enumerate(ext):
            vals[k] = call_closure(fn, np.ascontiguousarray(epts[k, :, :d]))
        out = np.empty(n, np.float64)
        _check(self.lib, self.lib.sdf_eval_points_extern_host(dt.handle, _dp(pts, _f64p), n, dim, _dp(vals, _f64p),
                                                              _dp(out, _f64p), self.precision))
        return out

    def estimate_bounds(self, sdf):
        """((x0, y0, z0), (x1, y1, z1)) of reference sdf/core.py:62-82 in one launch; None for a model with user
        closures (the caller then runs the reference's loop around eval_grid)"""
        dt = self.tape_for(sdf)
        if dt.tape.externs:
            return None
        out = np.zeros(6, np.float64)
        lib = self.lib
        if lib.sdf_estimate_bounds(dt.handle, _dp(out, _f64p), self.precision) != 0:
            msg = (lib.sdf_last_error() or b'').decode()
            if msg.startswith('zero-size array'):
                raise ValueError(msg)                       # what np.argwhere(...).max(axis=0) raises in the reference
            if 'barrier' in msg:
                return None                                 # (the caller runs the reference's loop around eval_grid)
            raise SdfHipError(msg)
        return (tuple(out[:3]), tuple(out[3:]))

    def eval_grid(self, sdf, X, Y, Z):
        dt = self.tape_for(sdf)
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        if dt.tape.externs:
            G = np.stack(np.meshgrid(X, Y, Z, indexing='ij'), axis=-1).reshape(-1, 3)
            return self._eval_points_hybrid(dt, np.ascontiguousarray(G)).reshape(len(X), len(Y), len(Z))
        out = np.empty((len(X), len(Y), len(Z)), np.float64)
        if out.size:
            _check(self.lib, self.lib.sdf_eval_grid_host(dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y),
                                                         _dp(Z, _f64p), len(Z), _dp(out, _f64p), self.precision))
        return out

    # -- meshing --
    def marching_cubes(self, volume):
        """soup (3T,3) float32 in volume index coordinates of a host volume
        (drop-in for reference sdf/core.py:16-18 `_marching_cubes`; raises nothing on an empty
        result, returns a (0,3) array)"""
        vol = np.ascontiguousarray(volume, dtype=np.float32)
        if vol.ndim != 3:
            raise ValueError('Input volume should be a 3D numpy array.')
        cells = max(1, (max(vol.shape[0], 1) - 1) * (max(vol.shape[1], 1) - 1) * (max(vol.shape[2], 1) - 1))
        cap = min(5 * cells, max(4096, 2 * cells))
        while True:
            out = np.empty((cap, 9), np.float32)
            nt = _c_i64(0)
            _check(self.lib, self.lib.sdf_marching_cubes_host(self.ctx, _dp(vol, _f32p), vol.shape[0], vol.shape[1],
                                                              vol.shape[2], _dp(out, _f32p), cap, ctypes.byref(nt)))
            if nt.value <= cap:
                return out[:nt.value].reshape(-1, 3)
            cap = nt.value

    def mesh_level_set(self, points, triangles, voxel_size, half_width_voxels):
        """the narrow-band signed-distance grid of a triangle mesh (sdf_mesh_level_set_host; what OpenVDB's
        createLevelSetFromPolygons + copyToArray give the reference's `Mesh.sdf`): returns
        (ijk0, A) with A the float32 values of the voxels ijk0 + [0, A.shape), voxel (i, j, k) at (i, j, k) * voxel_size.
        Raises ValueError, before any device work, for an empty mesh, an index out of range, a non-finite point,
        voxel_size <= 0 or a work grid larger than the device memory allows."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        tri = np.asarray(triangles)
        if pts.ndim != 2 or pts.shape[1] != 3 or tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError('points must be (V, 3) and triangles (T, 3), got %s and %s' % (pts.shape, tri.shape))
        if len(pts) == 0 or len(tri) == 0:
            raise ValueError('empty mesh: %d points, %d triangles' % (len(pts), len(tri)))
        if not np.all(np.isfinite(pts)):
            raise ValueError('the mesh has non-finite points')
        if tri.min() < 0 or tri.max() >= len(pts):
            raise ValueError('triangle indices must lie in [0, %d), got %d .. %d' % (len(pts), tri.min(), tri.max()))
        vs = float(voxel_size)
        if not (vs > 0 and np.isfinite(vs)):
            raise ValueError('voxel_size must be positive, got %r' % voxel_size)
        tri = np.ascontiguousarray(tri, dtype=np.int32)
        hw = int(half_width_voxels)
        # the work grid bounds the result: one call in the usual case
        lo = np.floor(pts.min(axis=0) / vs) - hw - 1
        hi = np.ceil(pts.max(axis=0) / vs) + hw + 1
        cap = int(min(np.prod(hi - lo + 1), 1 << 28))
        ijk0, dims = (_c_i64 * 3)(), (_c_i64 * 3)()
        while True:
            out = np.empty(cap, np.float32)
            _check(self.lib, self.lib.sdf_mesh_level_set_host(self.ctx, _dp(pts, _f64p), len(pts), _dp(tri, ctypes.POINTER(ctypes.c_int32)),
                                                              len(tri), vs, hw, ijk0, dims, _dp(out, _f32p), cap))
            n = int(np.prod(list(dims)))
            if n == 0:
                raise ValueError('no voxel lies within the narrow band of this mesh')
            if n <= cap:
                return np.array(list(ijk0), dtype=np.int64), out[:n].reshape(tuple(dims))
            cap = n

    def distance_texture(self, mask):
        """the signed exact Euclidean distance texture of a 2-D boolean mask, in pixels (sdf_distance_texture_host; what two
        scipy distance_transform_edt calls give the reference's `text` / `image`): float64 of the
        mask's shape, -sqrt(D) where the mask is True and +sqrt(D) elsewhere, D the integer squared distance to the
        nearest pixel of the other class.  Raises ValueError, before any device work, for a mask that is not 2-D, is
        empty, is too large or whose pixels are all of one class."""
        a = np.asarray(mask)
        if a.ndim != 2:
            raise ValueError('the mask must be 2-D, got shape %s' % (a.shape,))
        if a.size == 0:
            raise ValueError('empty mask: shape %s' % (a.shape,))
        a = np.ascontiguousarray(a != 0, dtype=np.uint8)
        out = np.empty(a.shape, np.float64)
        _check(self.lib, self.lib.sdf_distance_texture_host(self.ctx, _dp(a, _u8p), a.shape[0], a.shape[1], _dp(out, _f64p)))
        return out

    def render_buffers(self, sdf, frame, width, height, t_near=0.0, t_far=1e9, hit_eps=1e-4, step_scale=1.0, normal_eps=1e-4,
                       max_steps=256, refine=8):
        """the sphere-traced buffers of a model (sdf_render_host, csrc/sdf_render.hip): a dict of `depth`
        (height, width) float64 -- the hit's ray parameter, +inf for a miss --, `normal` (height, width, 3) float64, `steps`
        (height, width) int32 and `status` (height, width) uint8 (1 hit, 0 miss).  frame: 18 doubles o0, ou, ov, c, du, dv
        (sdf_amd/render.py `camera` makes one).  Raises ValueError, before any device work, for what the entry point refuses
        (include/sdf_hip.h), for a model with user closures and for a context in float32 precision."""
        dt, ev = self._probe_tape(sdf, 'render_buffers traces')
        if ev:
            raise ValueError('render_buffers cannot trace a model with user closures: every step of every ray would need a host round trip')
        frame = np.ascontiguousarray(frame, dtype=np.float64).reshape(-1)
        if frame.size != 18:
            raise ValueError('the ray frame has 18 numbers (o0, ou, ov, c, du, dv), got %d' % frame.size)
        w, h = int(width), int(height)
        if w < 1 or h < 1 or w * h > 1 << 26:
            raise ValueError('image of %d x %d: the sides must be positive and the pixels at most 2^26' % (w, h))
        params = np.array([t_near, t_far, hit_eps, step_scale, normal_eps], dtype=np.float64)
        out = {'depth': np.empty((h, w), np.float64), 'normal': np.empty((h, w, 3), np.float64), 'steps': np.empty((h, w), np.int32),
               'status': np.empty((h, w), np.uint8)}
        _check(self.lib, self.lib.sdf_render_host(dt.handle, _dp(frame, _f64p), w, h, _dp(params, _f64p), int(max_steps), int(refine),
                                                  _dp(out['depth'], _f64p), _dp(out['normal'], _f64p),
                                                  _dp(out['steps'], ctypes.POINTER(ctypes.c_int32)), _dp(out['status'], _u8p)))
        return out

    def generate(self, sdf, X, Y, Z, batch_size=32, sparse=True, shard=(0, 1), out_ptr=None, out_cap=0, wait=True, records=False):
        """mesh the grid X x Y x Z.  records=True (one device, the whole work list, no output buffer): for a
        caller who wants the soup on the HOST -- the triangles are kept as 16-byte records and `mesh.points(workers)`
        expands them on host threads (`sdf_generate_records`).  With out_ptr / out_cap (device memory for 9 * out_cap float64)
        the ordered soup is gathered into it inside the same submission (`mesh.emitted` tells
        whether it fitted); otherwise it stays in the mesh until `points()` / `emit_device()`.
        wait=False (needs out_ptr): the call is only enqueued; `mesh.wait()` -- or any read of the
        mesh -- collects it, so a caller can submit the next job while this one runs."""
        dt = self.tape_for(sdf)
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        h = _vp()
        emitted = ctypes.c_int(0)
        if dt.tape.externs:
            if out_ptr or not wait:
                raise ValueError('a model with user closures is meshed through the host callback path: no output '
                                 'buffer, no asynchronous submission')
            return self._generate_field(dt, X, Y, Z, batch_size, sparse, shard)
        if not wait:
            if not out_ptr:
                raise ValueError('generate(wait=False) needs an output buffer (out_ptr / out_cap)')
            _check(self.lib, self.lib.sdf_generate_to_device_async(
                dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z), int(batch_size),
                1 if sparse else 0, int(shard[0]), int(shard[1]), self.precision, _vp(out_ptr), int(out_cap),
                ctypes.byref(h)))
            m = Mesh(self, h)
            m._tape = dt
            m.emitted = None          # unknown until wait()
            return m
        if records and not out_ptr and tuple(shard) == (0, 1):
            _check(self.lib, self.lib.sdf_generate_records(dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y),
                                                           _dp(Z, _f64p), len(Z), int(batch_size), 1 if sparse else 0,
                                                           self.precision, ctypes.byref(h)))
        elif out_ptr:
            _check(self.lib, self.lib.sdf_generate_to_device(
                dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z), int(batch_size),
                1 if sparse else 0, int(shard[0]), int(shard[1]), self.precision, _vp(out_ptr), int(out_cap),
                ctypes.byref(emitted), ctypes.byref(h)))
        else:
            _check(self.lib, self.lib.sdf_generate(dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y),
                                                   _dp(Z, _f64p), len(Z), int(batch_size), 1 if sparse else 0,
                                                   int(shard[0]), int(shard[1]), self.precision, ctypes.byref(h)))
        m = Mesh(self, h)
        m._tape = dt          # keep the device tape alive as long as the mesh
        m.emitted = bool(emitted.value)
        return m

    def generate_dual(self, sdf, X, Y, Z, eps, reg=1e-3, batch_size=32, parts=False):
        """dual-contour the field on the dense grid X x Y x Z (sdf_generate_dual, csrc/sdf_dual.hip; defined
        by tests/dual_ref.py and reproduced bit for bit): one vertex in every grid cell that the surface crosses, placed by the
        quadric of the field's tangent planes at the cell's edge crossings (normals by central differences of step eps, the
        system regularised by reg towards the crossings' mean, the vertex clamped to its cell), two triangles per crossing edge.
        Returns a `Mesh` that owns its float64 soup and serves every reader; `mesh.dual_stats` holds the eight counters
        (crossings, cells, triangles, open_edges, nonfinite_edges, clamped, mean_fallback, flat) and `mesh.stats()` counts, as
        nonempty / empty, the blocks of batch_size^3 cells that hold / do not hold a vertex (batch_size steers nothing else).
        parts=True: `mesh.dual_parts` is the dict of points, normals (crossings x 3), vertices (cells x 3) and cells
        (triangles x 3 int64, indices into vertices) on the host.  Raises ValueError, before any device work, for an eps that is
        not positive and finite, a reg that is negative or not finite, an axis that is not finite, 2^31 or more samples, an engine in
        float32 precision and a model with user closures (the normals kernel serves neither)."""
        from .dual import STAT_KEYS, check_axes, check_params
        eps, reg = check_params(eps, reg)
        X, Y, Z = check_axes(X, Y, Z)
        dt = self._probe_tape(sdf, 'generate_dual contours the field')[0]
        h, p = _vp(), _vp()
        counters = np.zeros(8, np.int64)
        _check(self.lib, self.lib.sdf_generate_dual(self.ctx, dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z),
                                                    eps, reg, int(batch_size), ctypes.byref(h), _dp(counters, ctypes.POINTER(_c_i64)),
                                                    ctypes.byref(p) if parts else None))
        m = Mesh(self, h)
        m._tape = dt          # keep the device tape alive as long as the mesh
        m.emitted = False
        m.dual_stats = dict(zip(STAT_KEYS, (int(v) for v in counters)))
        if parts:
            try:
                c, k, t = (m.dual_stats[key] for key in ('crossings', 'cells', 'triangles'))
                got = {'points': np.zeros((c, 3), np.float64), 'normals': np.zeros((c, 3), np.float64),
                       'vertices': np.zeros((k, 3), np.float64), 'cells': np.zeros((t, 3), np.int64)}
                _check(self.lib, self.lib.sdf_dual_parts_fetch(p, _dp(got['points'], _f64p), _dp(got['normals'], _f64p), _dp(got['vertices'], _f64p),
                                                               _dp(got['cells'], ctypes.POINTER(_c_i64))))
                m.dual_parts = got
            finally:
                self.lib.sdf_dual_parts_destroy(p)
        return m


    def skip_kinds(self, sdf, X, Y, Z, batch_size, b_begin, b_end, kinds_ptr):
        """`_skip` for batches [b_begin, b_end): 0 / 255 into the caller's device buffer (one byte per batch of the grid)"""
        dt = self.tape_for(sdf)
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        _check(self.lib, self.lib.sdf_skip_kinds(dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z),
                                                 int(batch_size), int(b_begin), int(b_end), self.precision, _vp(kinds_ptr)))

    def generate_from_kinds(self, sdf, X, Y, Z, batch_size, kinds_ptr, shard=(0, 1)):
        """`generate` (sparse) with the skip test's verdicts already on the device (skip_kinds)"""
        dt = self.tape_for(sdf)
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        h = _vp()
        _check(self.lib, self.lib.sdf_generate_from_kinds(dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z),
                                                          int(batch_size), int(shard[0]), int(shard[1]), self.precision,
                                                          _vp(kinds_ptr), ctypes.byref(h)))
        m = Mesh(self, h)
        m._tape = dt
        m.emitted = False
        return m

    # -- the multi-GPU exchange unit (sdf_amd/dist.py) --
    SLAB_HEADER = ('n_tris', 'n_items', 'overflow', 'n_empty', 'n_nonempty', 'n_eval_voxels', 'n_ambiguous_cells',
                   'n_sampled_voxels', 'n_pruned_instrs', 'n_work_total')      # int64[16] at the head of a slab

    def slab_bytes(self, cap_items, cap_tris):
        return int(self.lib.sdf_slab_bytes(int(cap_items), int(cap_tris)))

    def generate_compact(self, sdf, X, Y, Z, batch_size, sparse, shard, slab_ptr, cap_items, cap_tris):
        """mesh this rank's shard into a slab in caller-owned device memory (enqueue only; the returned mesh
        keeps the call's device buffers alive until it is closed)"""
        dt = self.tape_for(sdf)
        X, Y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, Z))
        h = _vp()
        _check(self.lib, self.lib.sdf_generate_compact_async(
            dt.handle, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y), _dp(Z, _f64p), len(Z), int(batch_size),
            1 if sparse else 0, int(shard[0]), int(shard[1]), self.precision, _vp(slab_ptr), int(cap_items), int(cap_tris),
            ctypes.byref(h)))
        m = Mesh(self, h)
        m._tape = dt
        m.emitted = None
        return m

    def adopt_soup(self, device_ptr, n_triangles):
        """a Mesh over a float64 soup that already sits in device memory (n_triangles x 9 doubles, the caller's: it must
        stay alive and complete while the Mesh is used): STL records, weld and host copies then run on it like on a soup
        the library generated -- the gathered soup of a multi-GPU step"""
        h = _vp()
        _check(self.lib, self.lib.sdf_mesh_adopt_soup(self.ctx, _vp(int(device_ptr)), int(n_triangles), ctypes.byref(h)))
        return Mesh(self, h)

    def expand_slabs(self, slab_ptrs, cap_items, cap_tris, out_ptr, out_cap):
        """gathered slabs (device pointers, final order) -> ordered float64 soup at out_ptr (enqueue only)"""
        arr = (_vp * len(slab_ptrs))(*[_vp(int(p)) for p in slab_ptrs])
        _check(self.lib, self.lib.sdf_expand_slabs(self.ctx, arr, len(slab_ptrs), int(cap_items), int(cap_tris),
                                                   _vp(out_ptr), int(out_cap)))

    def _generate_field(self, dt, X, Y, Z, batch_size, sparse, shard):
        """`generate` for a model with user closures: the library drives the reference's batch loop and asks
        this callback for f(P) of the skip test and of every surviving batch (sdf_generate_field)"""
        failure = []

        def field(_user, p_pts, n, p_out):
            try:
                P = np.ctypeslib.as_array(p_pts, shape=(n, 3))
                np.ctypeslib.as_array(p_out, shape=(n,))[:] = self._eval_points_hybrid(dt, P)
                return 0
            except BaseException as e:      # (an exception cannot cross the C frames: it is re-raised below)
                failure.append(e)
                return 1

        cb = FIELD_FN(field)
        h = _vp()
        rc = self.lib.sdf_generate_field(self.ctx, ctypes.cast(cb, _vp), None, _dp(X, _f64p), len(X), _dp(Y, _f64p), len(Y),
                                         _dp(Z, _f64p), len(Z), int(batch_size), 1 if sparse else 0, int(shard[0]),
                                         int(shard[1]), ctypes.byref(h))
        if failure:
            raise failure[0]
        _check(self.lib, rc)
        m = Mesh(self, h)
        m._tape = dt
        m.emitted = False
        return m


_engines = {}


def get_engine(device=None):
    if device is None:
        device = int(os.environ.get('SDF_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    eng = _engines.get(device)
    if eng is None:
        eng = _engines[device] = Engine(device)
    return eng


def evaluate(sdf, p):
    """f(p) on the device -> (N,) float64 (reference sdf/d3.py:24-25 reshapes to (N,1))"""
    return get_engine().eval_points(sdf, p)
