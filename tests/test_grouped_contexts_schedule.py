"""Grouped contexts (``vf_set_contexts``) in the persistent schedule, on the CPU: the ASan / UBSan host build of
the engine with the driver ``tools/sanitize/host_selftest_grouped.cc``.  ``vf_selftest_schedule`` re-checks every pointer of
every phase of a grouped rollout - the per-row context buffers with their row strides and view offsets among them - against
the handle's allocations, for one and two views, one to three context frames, every compositing table and batches below
and at ``max_batch``; a grouped schedule shares nothing; ``vf_set_context`` brings the broadcast schedule back; and every
refusal of the two entries is refused with the handle left as it was."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.slow


def test_grouped_schedules_pass_the_host_self_test():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc not available')
    proc = subprocess.run(['bash', os.path.join(REPO, 'tools', 'sanitize', 'build_and_run_grouped.sh')],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0 and 'HOST SELFTEST (grouped contexts) OK' in proc.stdout, proc.stdout[-4000:]
    assert 'FAILED' not in proc.stdout and 'runtime error' not in proc.stdout and 'AddressSanitizer' not in proc.stdout
    rows = re.findall(r'^  grouped \S+ nd \d+ nctx \d+ ncam (\d+) spec (\d+)  \d+ x \d+ of \d+ rows: (\d+) items \(broadcast (\d+)\)$',
                      proc.stdout, re.M)
    assert len(rows) == 16 and {r[1] for r in rows} == set('01234') and {r[0] for r in rows} == {'1', '2'}
    assert all(int(g) >= int(b) for _, _, g, b in rows)
    # two context frames: the context steps are rolled per row, so the grouped schedule is strictly the larger one
    assert any(int(g) > int(b) for _, _, g, b in rows)
