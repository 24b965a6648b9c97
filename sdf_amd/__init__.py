"""sdf_amd -- MI355X-native drop-in for the fogleman/sdf sampling + meshing path.

``from sdf_amd import *`` (or ``from sdf import *`` through the alias package at the repo
root) exposes the same names as the reference package (reference sdf/__init__.py:1-27):
the 2-D / 3-D modelling API, the easing module, ``generate / save / sample_slice /
show_slice`` and ``write_binary_stl``.  Models are lowered to an op tape and sampled and
meshed by hand-written HIP kernels (sdf_amd/csrc); there is no CPU evaluation path for the library's own
nodes.  A user-written closure (a function decorated with ``@sdf3`` / ``@op3`` / ``@sdf2`` that returns NumPy
code, reference README.md:258-295) stays the user's code and runs on the host; everything around it runs on
the device.
"""
from . import d2, d3, ease

from .util import *

from .d2 import *

from .d3 import *

from .mesh import Mesh

from .text import (
    measure_image,
    measure_text,
    image,
    text,
)

from .core import (
    generate,
    generate_mesh,   # (not in the reference: the indexed mesh with the field's normals)
    save,
    sample_slice,
    show_slice,
)

from .stl import (
    write_binary_stl,
)

from .render import render   # (not in the reference: sphere-traced previews)
from .measure import measure   # (not in the reference: volume, area, inertia and the edge census on the device, section 4g)
from .thickness import thickness, Thickness   # (not in the reference: the wall thickness at the vertices of a mesh, probed on the device, section 4l)
from .curvature import curvature, curvature_of_soup, Curvature   # (not in the reference: mean, Gaussian and principal curvature of the field at the vertices of a mesh, probed on the device, section 4t)
from .dual import dual_of_grid   # (not in the reference: dual contouring of the field -- a mesh with sharp creases, `dual=` of everything that meshes, section 4u)
from .deviation import deviation, deviation_of_soup, Deviation  # (not in the reference: a mesh held to the field -- per-triangle deviation, vertices snapped back, section 4q)
from .shells import shells, measure_shells, Shells   # (not in the reference: the connected shells of a mesh, kept or dropped on the device, section 4h)
from .overhang import overhangs, overhangs_of_mesh, overhangs_soup, sphere_directions, Overhangs   # (not in the reference: build directions rated on the device, section 4n)
from .supports import supports, supports_of_mesh, supports_soup, Supports   # (not in the reference: support rays traced through the field, the true support volume of a build direction, section 4o)
