"""Static checks of the frames-only kernels (``vf_config.ndesig`` 0; csrc/vf_small_kernels.h, vf_fused_top.h,
vf_persistent.h) in the gfx950 code object, read the way tests/test_kernel_lint_dna.py reads it: every frames-only kernel
exists exactly once per compositing mode under a name of its own, spills no VGPR and keeps scratch <= 128 B (the bound of
the ND = 1..4 instances); the production kernel keeps its four spill-free instances; the barrier lint has no pending finding.
Resource metadata and symbol names only."""
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


# (mangled-name pattern, instances): the persistent rollouts, one per compositing mode, and the per-layer compositing kernels -
# CDNA with ten kernel slots (arch 0 / 1) and with six (arch 2), appearance flow, DNA
KERNELS = [(r'_ZN2vf21rollout_frames_kernelE\w+', 1), (r'_ZN2vf26rollout_flow_frames_kernelE\w+', 1),
           (r'_ZN2vf25rollout_dna_frames_kernelE\w+', 1), (r'_ZN2vf23composite_frames_kernelILi\d+E\w+', 2),
           (r'_ZN2vf28composite_flow_frames_kernelE\w+', 1), (r'_ZN2vf27composite_dna_frames_kernelE\w+', 1)]


@pytest.mark.parametrize('pattern,count', KERNELS)
def test_frames_only_kernels_exist_once_without_spills_and_with_little_scratch(assembly, pattern, count):
    kernels = _metadata(assembly, pattern)
    assert len(kernels) == count, sorted(kernels)
    for name, md in kernels.items():
        print(name, md)
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)
    if count == 2:
        assert sorted(int(re.search(r'ILi(\d+)E', n).group(1)) for n in kernels) == [6, 10]


def test_the_rollout_kernels_carry_frames_only_bodies_of_their_own(assembly):
    # out-of-line bodies: the stand-alone compositing tiles (CDNA plain / first frame / public decoder / six kernels; flow; DNA)
    # and the fused tops (conv_tile_call with the five frames-only epilogues 32 .. 36)
    labels = [l for l in assembly if re.match(r'^_ZN2vf\w+:', l)]
    assert len([l for l in labels if 'composite_frames_tile_call' in l]) == 4, labels
    assert len([l for l in labels if 'composite_flow_frames_tile_call' in l]) == 1
    assert len([l for l in labels if 'composite_dna_frames_tile_call' in l]) == 1
    fused = sorted(int(m.group(1)) for l in labels for m in [re.match(r'^_ZN2vfL14conv_tile_callILi4ELi(\d+)ELi1EEE', l)] if m)
    assert [e for e in fused if e >= 32] == [32, 33, 34, 35, 36], fused
    # no instance of a template that is counted per designated-pixel count was made for zero
    assert not [l for l in labels if re.search(r'(rollout_\w+_kernel|composite_\w*kernel|tile_call|ew_\w+_call)ILi0E', l)]


def test_production_kernel_keeps_four_spill_free_instances(assembly):
    kernels = _metadata(assembly, r'_ZN2vf25rollout_persistent_kernelILi\dE\w+')
    assert len(kernels) == 4
    for name, md in kernels.items():
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_barrier_lint_is_clean(assembly):
    import lint_barriers
    assert not [f for f in lint_barriers.lint(assembly) if f['pending']]
    assert lint_barriers.scheduler_barrier_is_guarded(assembly) == []
