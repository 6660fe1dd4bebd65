"""Pad skip (vf_conv_gsplit.h): the gate-split conv-LSTM tile leaves out the kernel rows of row blocks that read only zero
padding.  The skipped products are 0 x w, so every output must keep its bits: the same seeded rollouts (flagship plan,
small batches, 48 x 64 with row blocks below the image, two views, one context frame, arch 1 / 2 / 3) run in one child
with VF_PAD_SKIP=0 and in one with the default, and the frames, distributions, states, scores and elite indices are
compared bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, tag, pad_skip):
    env = dict(os.environ)
    env.pop('VF_PAD_SKIP', None)
    if pad_skip is not None:
        env['VF_PAD_SKIP'] = pad_skip
    out = str(tmp_path / ('%s.npz' % tag))
    proc = subprocess.run([sys.executable, '-m', 'tests.helpers.pad_skip_worker', out], cwd=REPO, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return np.load(out)


def test_pad_skip_is_bit_identical(tmp_path):
    full = _run(tmp_path, 'full', '0')
    skip = _run(tmp_path, 'skip', None)
    assert sorted(full.files) == sorted(skip.files)
    assert any(k.endswith('/predicted_frames') for k in full.files)
    for k in full.files:
        a, b = full[k], skip[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), '%s differs with pad skip on' % k
