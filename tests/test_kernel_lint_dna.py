"""Static checks of the DNA compositing kernels (csrc/vf_small_kernels.h, vf_fused_top.h, vf_persistent.h) in the gfx950 code
object, read the way tests/test_kernel_lint.py reads them: the four rollout_dna_kernel and the four composite_dna_kernel
instances exist, spill no VGPR and keep scratch <= 128 B; the production kernel keeps its four spill-free instances; the
barrier lint has no pending finding."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))

pytestmark = pytest.mark.slow


@pytest.fixture(scope='module')
def assembly():
    import lint_barriers
    if not (os.path.exists('/opt/rocm/bin/hipcc') or any(
            os.path.exists(os.path.join(d, 'hipcc')) for d in os.environ.get('PATH', '').split(os.pathsep))):
        pytest.skip('hipcc not available')
    return lint_barriers.device_assembly()


def _metadata(assembly, pattern):
    text = '\n'.join(assembly)
    out = {}
    for m in re.finditer(r'\.name:\s+(%s)\n(.*?)\.wavefront_size' % pattern, text, re.S):
        blk = m.group(0)
        out[m.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
                           for k in ('vgpr_spill_count', 'private_segment_fixed_size', 'vgpr_count')}
    return out


@pytest.mark.parametrize('pattern', [r'_ZN2vf18rollout_dna_kernelILi\dE\w+', r'_ZN2vf20composite_dna_kernelILi\dE\w+'])
def test_dna_kernels_have_no_spills_and_little_scratch(assembly, pattern):
    kernels = _metadata(assembly, pattern)
    assert len(kernels) == 4, sorted(kernels)
    for name, md in kernels.items():
        print(name, md)
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_the_rollout_kernels_carry_the_dna_bodies(assembly):
    # the fused top and the compositing tile of a dna engine are out-of-line bodies of rollout_dna_kernel: one
    # composite_dna_tile_call per designated-pixel count
    bodies = [l for l in assembly if re.match(r'^_ZN2vf\w*composite_dna_tile_call\w*:', l)]
    assert len(bodies) == 4, bodies


def test_production_kernel_keeps_four_spill_free_instances(assembly):
    kernels = _metadata(assembly, r'_ZN2vf25rollout_persistent_kernelILi\dE\w+')
    assert len(kernels) == 4
    for name, md in kernels.items():
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_barrier_lint_is_clean(assembly):
    import lint_barriers
    assert not [f for f in lint_barriers.lint(assembly) if f['pending']]
