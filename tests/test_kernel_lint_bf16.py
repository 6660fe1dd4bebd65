"""Static checks of the plain-bf16 conv-LSTM tile (csrc/vf_conv_bf16.h) in the gfx950 code object, read the way
tests/test_kernel_lint.py reads them: the stand-alone kernel and the persistent kernels that carry the tile as an out-of-line
body spill no VGPR and keep scratch <= 128 B, and every loop-head barrier of the new tile waits for its LDS stores."""
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


def test_standalone_kernel_has_no_spills_and_no_scratch(assembly):
    kernels = _metadata(assembly, r'_ZN2vf21conv_lstm_bf16_kernel\w+')
    assert len(kernels) == 1, sorted(kernels)
    for name, md in kernels.items():
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def test_persistent_kernels_carry_the_tile_without_spills(assembly):
    # the tile is an out-of-line body of every rollout_persistent_kernel instance: its symbol is in the listing ...
    bodies = [l for l in assembly if re.match(r'^_ZN2vf\w*lstm_bf16_tile_call\w*:', l)]
    assert len(bodies) == 1, bodies
    # ... and the instances that call it still spill nothing
    kernels = _metadata(assembly, r'_ZN2vf25rollout_persistent_kernelILi\dE\w+')
    assert len(kernels) == 4
    for name, md in kernels.items():
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['private_segment_fixed_size'] <= 128, (name, md)


def _function_spans(assembly):
    spans, func, start = [], None, 0
    for k, l in enumerate(assembly):
        m = re.match(r'^(_Z\w+):', l)
        if m:
            if func:
                spans.append((func, start, k))
            func, start = m.group(1), k
    if func:
        spans.append((func, start, len(assembly)))
    return spans


def test_barrier_lint_is_clean_on_the_new_tile(assembly):
    import lint_barriers
    ours = [(f, a, b) for f, a, b in _function_spans(assembly) if 'conv_lstm_bf16_kernel' in f or 'lstm_bf16_tile_call' in f]
    assert len(ours) == 2, [f for f, _, _ in ours]
    # no loop-head barrier of the tile is listed at all: each sits behind the explicit `s_waitcnt lgkmcnt(0)` of the header
    findings = [f for f in lint_barriers.lint(assembly) if any(f['func'] == name for name, _, _ in ours)]
    assert findings == [], findings
    for name, a, b in ours:
        body = assembly[a:b]
        assert any('v_mfma_f32_32x32x16_bf16' in l for l in body), name
        assert sum('s_barrier' in l for l in body) >= 3, name
    # the whole code object stays clean as well
    assert not [f for f in lint_barriers.lint(assembly) if f['pending']]
