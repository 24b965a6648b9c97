"""What the compiler makes of the three one-pass three-sample variants of k_mesh, without a GPU: spilled scalar registers under a
ceiling, spilled vector registers and scratch no higher than before the scalar state of a round was cut down, four waves per SIMD.

The figures come from the compiler's own `kernel-resource-usage` remarks through tools/kernel_resources.sh (a cross-compile; no
instruction text is read).  A compile of the whole family takes most of a minute, so each variant is instantiated alone through
tests/native/mesh_resources_probe.hip -- the three compiles run side by side, a few seconds together.

A spilled scalar is a lane write behind a wait state and a lane read where it is used: two issue slots that compute nothing, on a
kernel that is bound by instruction issue (profiles/r07a_scalar_spills.md).  The ceilings are what that change reached, rounded up
to the next multiple of 8 (it reached 50, 67 and 63 spilled scalars, from 156, 158 and 156): a change that brings the spills back fails here.  Vector spills and scratch:
the values of profiles/r06ak_kernel_resources.txt."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'            # (the compiler tools/kernel_resources.sh calls)
PROBE = os.path.join(ROOT, 'tests', 'native', 'mesh_resources_probe.hip')

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc: nothing to cross-compile with')

# register file as launch_mesh numbers it -> (NP, ND, NS), ceiling of spilled SGPRs, spilled VGPRs and scratch bytes per lane of r06ak
VARIANTS = {
    0: ((1, 1, 3), 56, 54, 304),
    1: ((2, 2, 3), 72, 82, 400),
    3: ((2, 4, 3), 64, 166, 448),
}


def compile_variant(file_no):
    env = dict(os.environ, MESH_SRC=PROBE)
    r = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'kernel_resources.sh'), 'double', '0', '-DPROBE_FILE=%d' % file_no],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith('k_mesh<')]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout, r.stderr)
    return lines[0]


@pytest.fixture(scope='module')
def table():
    with ThreadPoolExecutor(len(VARIANTS)) as pool:
        return dict(zip(VARIANTS, pool.map(compile_variant, VARIANTS)))


def field(line, name):
    return int(re.search(re.escape(name) + r': (\d+)', line).group(1))


@pytest.mark.parametrize('file_no', sorted(VARIANTS))
def test_one_pass_three_sample_variant(table, file_no):
    (n_p, n_d, n_s), sgpr_ceiling, vgpr_spill_r06ak, scratch_r06ak = VARIANTS[file_no]
    line = table[file_no]
    print(line)
    # the one-pass instantiation of this register file of the kernel a normal call launches (not k_mesh_prof)
    assert line.startswith('k_mesh<d,0,%d,%d,%d,1024,0>' % (n_p, n_d, n_s)), line
    assert sgpr_ceiling < 119                     # (what two trivial edits reached before this work began: the ceiling is below that)
    assert field(line, 'SGPRs Spill') <= sgpr_ceiling
    assert field(line, 'VGPRs Spill') <= vgpr_spill_r06ak
    assert field(line, 'ScratchSize [bytes/lane]') <= scratch_r06ak
    assert field(line, 'Occupancy [waves/SIMD]') == 4 and field(line, 'VGPRs') == 128
