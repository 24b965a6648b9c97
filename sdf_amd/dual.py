"""Dual contouring of the field: a mesh with sharp creases (not in the reference, whose meshes all come from
marching cubes).  `dual=` of the mesh pipeline and `dual_of_grid`; the device unit is csrc/sdf_dual.hip, the definition
tests/dual_ref.py."""
import numpy as np

DUAL_KEYS = ('eps', 'reg')
STAT_KEYS = ('crossings', 'cells', 'triangles', 'open_edges', 'nonfinite_edges', 'clamped', 'mean_fallback', 'flat')
DEFAULT_REG = 1e-3


def check_params(eps, reg):
    """(eps, reg) as floats, or ValueError: eps positive and finite, reg finite and not negative"""
    try:
        eps, reg = float(eps), float(reg)
    except (TypeError, ValueError):
        raise ValueError('dual: eps and reg are real numbers, got %r and %r' % (eps, reg))
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError('dual: eps must be positive and finite, got %r' % (eps,))
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError('dual: reg must be finite and not negative, got %r' % (reg,))
    return eps, reg


def check_dual_option(dual):
    """the `dual=` of the mesh pipeline: None for False / None (the call without it), else the dict of overrides (True: {}).  A dict
    may hold eps and reg; whatever it holds is checked here, before anything is meshed"""
    if dual is None or dual is False:
        return None
    if dual is True:
        return {}
    if not isinstance(dual, dict):
        raise ValueError('dual: True, False or a dict of %s, got %r' % (', '.join(DUAL_KEYS), dual))
    unknown = set(dual) - set(DUAL_KEYS)
    if unknown:
        raise ValueError('dual: unknown arguments %s' % sorted(unknown))
    check_params(dual.get('eps', 1.0), dual.get('reg', DEFAULT_REG))
    return dict(dual)


def dual_params(over, bounds):
    """the (eps, reg) of `engine.Engine.generate_dual` for a mesh within bounds: eps = the preview's normal_eps
    (`core.default_normal_eps`), reg = 1e-3 -- each overridden by the dict `over`"""
    from . import core
    par = {'eps': core.default_normal_eps(bounds), 'reg': DEFAULT_REG}
    par.update(over)
    return check_params(par['eps'], par['reg'])


def check_axes(X, Y, Z):
    """the three axes as contiguous float64 vectors, or ValueError: an axis value that is not finite, 2^31 or more samples"""
    axes = tuple(np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (X, Y, Z))
    for name, a in zip('XYZ', axes):
        if not np.isfinite(a).all():
            raise ValueError('dual: axis %s is not finite' % name)
    if len(axes[0]) * len(axes[1]) * len(axes[2]) >= 2 ** 31:
        raise ValueError('dual: 2^31 or more samples')
    return axes


def dual_of_grid(f, X, Y, Z, eps=None, reg=DEFAULT_REG):
    """(vertices (K, 3) float64, cells (T, 3) int64, stats): the model f dual-contoured on the grid X x Y x Z on the device, indexed --
    one vertex per grid cell that the surface crosses, so the vertex array is welded by construction -- with the eight counters
    of `engine.Engine.generate_dual` as stats.  eps: the step of the normals' central difference, default the preview's for the
    box the axes span; reg: the regularisation of the quadric towards the mean of a cell's crossings."""
    from . import core, engine
    X, Y, Z = check_axes(X, Y, Z)
    if eps is None:
        if min(len(X), len(Y), len(Z)) < 1:
            raise ValueError('dual: eps is needed for an empty axis')
        eps = core.default_normal_eps(((X[0], Y[0], Z[0]), (X[-1], Y[-1], Z[-1])))
    eps, reg = check_params(eps, reg)
    eng = engine.get_engine()
    mesh = eng.generate_dual(eng.tape_for(f), X, Y, Z, eps, reg, parts=True)
    try:
        return mesh.dual_parts['vertices'], mesh.dual_parts['cells'], dict(mesh.dual_stats)
    finally:
        mesh.close()
