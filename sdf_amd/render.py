"""Looking at a model without meshing it: sphere tracing on the device (csrc/sdf_render.hip).

    f.render('preview.png')                    # needs Pillow, and nothing else
    buf = render.render_buffers(f, 640, 480)   # depth / normal / steps / status, for a shading of your own
    img = render.shade(buf, buf['frame'])      # (h, w, 3) uint8, pure NumPy

`camera` makes the ray frame the kernel takes (18 doubles: o0, ou, ov, c, du, dv -- pixel (row j, column i) has the origin
(o0 + i ou) + j ov and the direction ((c + i du) + j dv) normalised), `render_buffers` runs the tracer, `shade` turns its
buffers into an image on the host and `render` does all three.  (The package attribute `sdf_amd.render` is the function;
this module is `importlib.import_module('sdf_amd.render')`.)"""
import numpy as np

DIRECTION = (1.0, -1.5, 1.0)     # the default view: from this side of the bounds' centre


def _unit(v, what):
    v = np.asarray(v, dtype=np.float64).reshape(3)
    n = np.sqrt(np.dot(v, v))
    if not (n > 0 and np.isfinite(n)):
        raise ValueError('%s has no direction: %r' % (what, tuple(v)))
    return v / n


def camera(bounds, width, height, eye=None, target=None, up=(0, 0, 1), fov=30.0, ortho=False):
    """(frame, t_near, t_far, radius) for an image of width x height pixels of the box `bounds` = ((x0, y0, z0), (x1, y1, z1)).

    radius is the half-diagonal of the bounds.  target defaults to their centre, eye to the point at radius / sin(fov / 2)
    from the target in direction (1, -1.5, 1): the bounding sphere then just fits the image's shorter side (fov, in degrees,
    is the field of view across that side).  An orthographic view (ortho=True) shows 2 * radius across the shorter side.
    t_near, t_far = |eye - centre| -+ radius, t_near clamped to 0: no ray meets the bounding sphere outside them."""
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError('image of %d x %d' % (w, h))
    if not (0 < fov < 180):
        raise ValueError('fov must lie in (0, 180) degrees, got %r' % (fov,))
    centre = (lo + hi) / 2
    radius = float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    if not (radius > 0 and np.isfinite(radius)):
        raise ValueError('the bounds %r have no extent' % (bounds,))
    half = np.radians(fov) / 2
    target = centre if target is None else np.asarray(target, dtype=np.float64).reshape(3)
    if eye is None:
        eye = target + _unit(DIRECTION, 'the default direction') * (radius / np.sin(half))
    eye = np.asarray(eye, dtype=np.float64).reshape(3)
    forward = _unit(target - eye, 'the view (eye == target)')
    side = np.cross(forward, np.asarray(up, dtype=np.float64).reshape(3))
    if np.dot(side, side) < 1e-24:                       # looking along `up`: any horizon will do
        side = np.cross(forward, (1.0, 0.0, 0.0) if abs(forward[0]) < 0.9 else (0.0, 1.0, 0.0))
    right = _unit(side, 'the horizon')
    upv = np.cross(right, forward)
    # pixel (j, i) sits at u = (i + 0.5 - w / 2) * s to the right of and v = (h / 2 - 0.5 - j) * s above the view axis
    s = (2 * radius if ortho else 2 * np.tan(half)) / min(w, h)
    corner = (0.5 - w / 2) * s * right + (h / 2 - 0.5) * s * upv
    zero = np.zeros(3)
    if ortho:
        frame = np.concatenate([eye + corner, s * right, -s * upv, forward, zero, zero])
    else:
        frame = np.concatenate([eye, zero, zero, forward + corner, s * right, -s * upv])
    dist = float(np.sqrt(np.dot(eye - centre, eye - centre)))
    return frame, max(0.0, dist - radius), dist + radius, radius


def directions(frame, width, height):
    """the unit ray directions of a frame, (height, width, 3)"""
    f = np.asarray(frame, dtype=np.float64).reshape(6, 3)
    j, i = np.mgrid[0:height, 0:width]
    d = f[3] + i[..., None] * f[4] + j[..., None] * f[5]
    return d / np.sqrt((d * d).sum(axis=-1, keepdims=True))


def render_buffers(sdf, width=1024, height=768, bounds=None, hit_eps=None, normal_eps=None, step_scale=1.0, max_steps=256, refine=8,
                   **camera_args):
    """trace `sdf` on the device: the dict of `Engine.render_buffers` (depth, normal, steps, status) plus the `frame` it was
    traced with and `t_near`, `t_far`, `radius`.  bounds default to the model's estimated bounds, hit_eps and normal_eps to
    1e-4 * radius; camera_args go to `camera` (eye, target, up, fov, ortho)."""
    from . import core, d2, engine
    if isinstance(sdf, d2.SDF2):
        raise TypeError('a 2-D model cannot be rendered: give it a thickness first, e.g. with .extrude()')
    if bounds is None:
        bounds = core._estimate_bounds(sdf)
    frame, t_near, t_far, radius = camera(bounds, width, height, **camera_args)
    hit_eps = 1e-4 * radius if hit_eps is None else hit_eps
    normal_eps = 1e-4 * radius if normal_eps is None else normal_eps
    out = engine.get_engine().render_buffers(sdf, frame, width, height, t_near=t_near, t_far=t_far, hit_eps=hit_eps, step_scale=step_scale,
                                             normal_eps=normal_eps, max_steps=max_steps, refine=refine)
    out.update(frame=frame, t_near=t_near, t_far=t_far, radius=radius)
    return out


def shade(buffers, frame, light=None, color=(0.35, 0.55, 0.85), background=(1, 1, 1), ambient=0.25):
    """(h, w, 3) uint8 from render buffers, on the host: a hit gets color * (ambient + (1 - ambient) * max(0, n . l)), a miss
    the background; l is the unit vector towards the light -- `light`, or by default a headlight (against each pixel's ray)"""
    status = np.asarray(buffers['status'])
    n = np.asarray(buffers['normal'], dtype=np.float64)
    h, w = status.shape
    if light is None:
        l = -directions(frame, w, h)
    else:
        l = np.broadcast_to(_unit(light, 'the light'), (h, w, 3))
    lambert = np.maximum(0.0, (n * l).sum(axis=-1))
    lit = (ambient + (1.0 - ambient) * lambert)[..., None] * np.asarray(color, dtype=np.float64)
    rgb = np.where((status == 1)[..., None], lit, np.asarray(background, dtype=np.float64))
    return np.rint(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


def render(sdf, path=None, light=None, color=(0.35, 0.55, 0.85), background=(1, 1, 1), ambient=0.25, **kw):
    """the shaded image of `sdf`, (h, w, 3) uint8; written to `path` with Pillow when one is given (kw: render_buffers)"""
    buf = render_buffers(sdf, **kw)
    img = shade(buf, buf['frame'], light=light, color=color, background=background, ambient=ambient)
    if path is not None:
        from PIL import Image
        Image.fromarray(img, 'RGB').save(path)
    return img
