#!/usr/bin/env python3
"""tests/golden/edt.npz: masks and the distance textures scipy gives for them -- `sdf_amd.text.distance_texture(mask)`, the
host path, i.e. two calls of scipy.ndimage.distance_transform_edt as in reference sdf/text.py:77-87 -- so that the NumPy
restatement (tests/edt_ref.py) stays pinned to scipy's bits where scipy is not installed.

    python tools/make_golden_edt.py

Needs scipy, Pillow and matplotlib (for its bundled DejaVuSans.ttf: the 'hello' mask is `text(font, 'Hello', points=64)`'s,
and a glyph raster depends on the FreeType build, so the mask itself is recorded).  Per case: `mask_<name>` (np.packbits),
`shape_<name>`, `tex_<name>` (float64).  Recorded with scipy 1.15.3."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import edt_ref  # noqa: E402

NAMES = ('r_37x53_50', 'r_53x37_10', 'r_1x200_50', 'r_200x1_30', 'r_17x130_02', 'r_131x19_98', 'single_true', 'single_false',
         'checkerboard', 'frame')


def main():
    T = importlib.import_module('sdf_amd.text')
    masks = {k: v for k, v in edt_ref.cases().items() if k in NAMES}
    masks['hello'] = edt_ref.rendered_mask(edt_ref.dejavu(), 'Hello', 64)
    out = {}
    for name, m in masks.items():
        out['mask_' + name] = np.packbits(m)
        out['shape_' + name] = np.array(m.shape, dtype=np.int64)
        out['tex_' + name] = T.distance_texture(m)
        print(name, m.shape, int(m.sum()), 'True pixels')
    np.savez_compressed(edt_ref.GOLDEN, **out)
    print(edt_ref.GOLDEN, os.path.getsize(edt_ref.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
