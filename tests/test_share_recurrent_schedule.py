"""Shared recurrent partial (vf_engine.hip, emit_rollout) in the persistent schedule, on the CPU: the host self-test
(tools/sanitize) builds and verifies the schedules of its shapes with the switch on, then the same binary runs with
VF_SHARE_RECURRENT=0.  The two runs may differ only where a conv-LSTM turns per-sample on a still shared recurrent input:
never with one context frame (not even at batches whose plans could consume a partial), never in the schedule of a cached
context (the partial is a cached shared unit), and at the flagship shape by exactly the partials' items."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.slow


def _items(text):
    """{(shape line, B, schedule variant): items} in the order the self-test prints them, per occurrence."""
    out = {}
    for m in re.finditer(r'^  (\S+ adim \d+ nd \d+ ncam \d+ prec \d+)  B=(\d+)\s+([^:]+): (\d+) items$', text, re.M):
        key = (m.group(1), int(m.group(2)), m.group(3))
        n = sum(1 for k in out if k[:3] == key)
        out[key + (n,)] = int(m.group(4))
    return out


def test_partials_are_emitted_only_where_the_recurrent_input_is_shared():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc not available')
    env = dict(os.environ)
    env.pop('VF_SHARE_RECURRENT', None)
    proc = subprocess.run(['bash', os.path.join(REPO, 'tools', 'sanitize', 'build_and_run.sh')], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0 and 'HOST SELFTEST OK' in proc.stdout, proc.stdout[-4000:]
    env['VF_SHARE_RECURRENT'] = '0'
    off = subprocess.run([os.path.join(REPO, 'build', 'vf_host_selftest')], env=env, cwd=REPO,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert off.returncode == 0 and 'HOST SELFTEST OK' in off.stdout, off.stdout[-4000:]
    on, own = _items(proc.stdout), _items(off.stdout)
    assert sorted(on) == sorted(own) and len(on) > 100
    for key in on:
        shape, B, variant, _ = key
        if variant.startswith('cached-context'):
            assert on[key] == own[key], key           # a cached context skips the partial like every shared unit
        else:
            assert on[key] >= own[key], key
    # one context frame: nothing is emitted.  At B = 1 / 7 / 16 (the self-test's first 64 x 64 shape) the 32-row plans could
    # not consume a partial anyway; the second shape of that name and batch (below: occurrence 1 of B = 200 / 125 / 25) has one
    # context frame at batches whose plans could - lstm1-4 read a shared h(0) at step 1 there - and must not differ either
    small = [k for k in on if k[0] == '64x64 adim 4 nd 1 ncam 1 prec 0' and k[1] in (1, 7, 16)]
    assert len(small) == 12 and all(on[k] == own[k] for k in small)
    ctx1 = [k for k in on if k[0] == '64x64 adim 4 nd 1 ncam 1 prec 0' and k[1] in (200, 125, 25) and k[3] == 1]
    assert len(ctx1) == 12 and all(on[k] == own[k] for k in ctx1)
    # the flagship (64 x 64, two context frames, 200 samples; occurrence 0): lstm5-7 at step 1 and lstm1-4 at step 2 - 8 tiles x 1 channel
    # group for the 32 x 32 layers (lstm1, 2, 7), 2 x 2 for the 16 x 16 ones (lstm3, 4, 6), one two-image tile x 4 for lstm5
    flag = ('64x64 adim 4 nd 1 ncam 1 prec 0', 200, 'full', 0)
    assert on[flag] - own[flag] == 3 * 8 + 3 * 4 + 4
    # 25 samples: only the layers whose plan is a 64- or 128-row gate-split tile get a partial
    assert on[(flag[0], 25, 'full', 0)] - own[(flag[0], 25, 'full', 0)] == 24
    # the 64 x 64 core of arch 1 and arch 2 at 128 x 128 (the self-test's first two exact-fp32 shapes of that size; arch 2
    # conditions every conv-LSTM on the action, so all seven turn per-sample at one step): the same 40 items
    big = '128x128 adim 12 nd 1 ncam 1 prec 0'
    assert on[(big, 125, 'full', 0)] - own[(big, 125, 'full', 0)] == 40
    assert on[(big, 125, 'full', 1)] - own[(big, 125, 'full', 1)] == 40
