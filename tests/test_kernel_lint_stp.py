"""Static checks of the STP kernels (csrc/vf_small_kernels.h, vf_fused_top.h, vf_persistent.h) in the gfx950 code object,
read the way tests/test_kernel_lint_dna.py reads them - from the code object's metadata only: the four rollout_stp_kernel and
the four composite_stp_kernel instances, the frames-only twins and stp_finalize_kernel exist, spill no VGPR and keep scratch
<= 128 B; the kernels of the other compositing modes keep their instance counts; the barrier lint has no pending finding."""
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


@pytest.mark.parametrize('pattern,count', [(r'_ZN2vf18rollout_stp_kernelILi\dE\w+', 4),
                                           (r'_ZN2vf20composite_stp_kernelILi\dE\w+', 4),
                                           (r'_ZN2vf25rollout_stp_frames_kernel\w+', 1),
                                           (r'_ZN2vf27composite_stp_frames_kernel\w+', 1),
                                           (r'_ZN2vf19stp_finalize_kernel\w+', 1)])
def test_stp_kernels_have_no_spills_and_little_scratch(assembly, pattern, count):
    kernels = _metadata(assembly, pattern)
    assert len(kernels) == count, sorted(kernels)
    for name, md in kernels.items():
        print(name, md)
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_the_rollout_kernels_carry_the_stp_bodies(assembly):
    # the compositing tile and the finish item of an stp engine are out-of-line bodies of rollout_stp_kernel: one
    # composite_stp_tile_call per designated-pixel count, one frames-only twin, one stp_finalize_call
    bodies = [l for l in assembly if re.match(r'^_ZN2vf\w*composite_stp_tile_call\w*:', l)]
    assert len(bodies) == 4, bodies
    assert len([l for l in assembly if re.match(r'^_ZN2vf\w*composite_stp_frames_tile_call\w*:', l)]) == 1
    # ... and so are its fused tops (the epilogues 37 .. 41 behind names of their own: conv_tile_call keeps its instances)
    assert len([l for l in assembly if re.match(r'^_ZN2vf\w*top_stp_tile_call\w*:', l)]) == 4
    assert len([l for l in assembly if re.match(r'^_ZN2vf\w*top_stp_frames_tile_call\w*:', l)]) == 1
    fused = [int(m.group(1)) for l in assembly for m in [re.match(r'^_ZN2vfL14conv_tile_callILi4ELi(\d+)ELi1EEE', l)] if m]
    assert not [e for e in fused if e >= 37], fused
    assert len([l for l in assembly if re.match(r'^_ZN2vf\w*stp_finalize_call\w*:', l)]) == 1


@pytest.mark.parametrize('pattern', [r'_ZN2vf25rollout_persistent_kernelILi\dE\w+', r'_ZN2vf19rollout_flow_kernelILi\dE\w+',
                                     r'_ZN2vf18rollout_dna_kernelILi\dE\w+'])
def test_the_other_rollout_kernels_keep_four_spill_free_instances(assembly, pattern):
    kernels = _metadata(assembly, pattern)
    assert len(kernels) == 4
    for name, md in kernels.items():
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_barrier_lint_is_clean(assembly):
    import lint_barriers
    assert not [f for f in lint_barriers.lint(assembly) if f['pending']]
