"""Shared recurrent partial (vf_engine.hip, emit_rollout): at the step at which a conv-LSTM turns per-sample it still reads
one shared h(s-1), so the gate sums of its recurrent chunks are computed once and every sample's item starts its
accumulators from them.  Storing and reloading fp32 sums and continuing the same fma chain must keep every bit: the same
seeded planning calls (64 x 64 and 48 x 64 with 1 / 3 / 25 / 200 samples, one to three context frames, two views, several
rollouts per context and a changed context, one launch per layer, arch 1 / 2) run in one child with VF_SHARE_RECURRENT=0
and in one with the default, and the frames, distributions, states and scores are compared bitwise.  The executed FLOPs the
engine counts for the first rollout of each case show that the default run did take the partial path where a plan can consume
it, and that nothing is emitted with one context frame or for the 32-row plans of the smallest batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, tag, share):
    env = dict(os.environ)
    env.pop('VF_SHARE_RECURRENT', None)
    if share is not None:
        env['VF_SHARE_RECURRENT'] = share
    out = str(tmp_path / ('%s.npz' % tag))
    proc = subprocess.run([sys.executable, '-m', 'tests.helpers.share_recurrent_worker', out], cwd=REPO, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return np.load(out)


def test_shared_recurrent_partial_is_bit_identical(tmp_path):
    own = _run(tmp_path, 'own', '0')
    shared = _run(tmp_path, 'shared', None)
    assert sorted(own.files) == sorted(shared.files)
    assert any('/predicted_frames' in k for k in own.files)
    # where the partial ran: fewer executed FLOPs (199 of 200 samples' recurrent sums gone) - and only there
    fewer = ('c64_m25', 'c64_m200', 'c48x64_m200', 'c64_ctx3_m25', 'c64_ctx3_m200', 'c64_m25_layers', 'c64_m200_layers',
             'savp_128_m125', 'savp2_128_m125')
    same = ('c64_m1', 'c64_m3', 'c48x64_m1', 'c48x64_m3', 'c48x64_ctx3_layers', 'c64_ctx1', 'c64_ctx1_m200')
    for name in fewer + same:
        a, b = float(own['meta/%s/flops' % name]), float(shared['meta/%s/flops' % name])
        print('%-20s executed FLOPs own %.6e shared %.6e' % (name, a, b))
        assert a > 0 and b > 0, name
        assert (b < a) if name in fewer else (b == a), (name, a, b)
    differ = []
    for k in own.files:
        if k.startswith('meta/'):
            continue
        a, b = own[k], shared[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.tobytes() != b.tobytes():
            differ.append(k)
    assert not differ, 'differs with the shared recurrent partial on: %s' % differ[:20]
