"""Bit identity of the frame scorer and the registration network across changes of their shared code (``csrc/vf_net_conv.h``,
``csrc/vf_engine_sidenet.inc``): sha256 digests of the raw float32 outputs for fixed inputs and seeded random weights,
compared with ``tests/golden/side_net_bits.json``.

The digests pin the summation order of the matrix-pipe layers (taps ascending, channel blocks ascending, K never split)
on the smallest shapes that reach every path of the shared core:

  scorer 16x32    c2 is one exactly full 32-position tile, c3 and c4 are tiles of 8 and 2 positions
  scorer 48x64    c3 has a partly filled last tile (48 = 32 + 16), c4 a single partly filled tile of 12 positions
                  (both towers of an embedding head with embed_dim 24 and ncam 2: Cin 3 and 6, a per-view weight stride)
  regnet 40x56 ch_mult 1 ncam 2    every layer has partly filled tiles, both tile widths occur, u3 has 16 channels in a
                                   32-wide tile, the pooled 16-wide tiles meet Win % 16 != 0
  regnet 64x112 ch_mult 4 ncam 1   d2 runs with two channel tiles per wave, pooling and a partly filled tile
  regnet 48x64 ch_mult 1 ncam 1    the shape of test_gpu_registration_net's own bit-identity test

The fixture is minted with the library of the commit BEFORE a change, never from the code under test: check that commit
out into a scratch directory, build it there, and run this module against that tree on a GPU,

    PYTHONPATH=<that tree> python tests/test_gpu_side_net_bits.py --mint tests/golden/side_net_bits.json

(the module uses only ``HipFrameScorer.embed`` and ``HipRegistrationNet.flow``).  An intended change of summation order is
the only reason to mint again; any other difference means the order changed by accident - fix the code, not the fixture.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'side_net_bits.json')

SCORER_CASES = [(16, 32), (48, 64)]                                 # H, W
REGNET_CASES = [(40, 56, 1, 2), (64, 112, 4, 1), (48, 64, 1, 1)]    # H, W, ch_mult, ncam


def _digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def scorer_digests(H, W):
    """{tower: digest} of ``embed`` on 3 images for both towers of an embedding head (embed_dim 24, ncam 2)."""
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    scorer = HipFrameScorer('', dict(image_height=H, image_width=W, ncam=2, head='embedding', embed_dim=24, max_frames=3,
                                     seed=5, bias_scale=0.2)).restore()
    rs = np.random.RandomState(1000 + H + W)
    out = {}
    for tower, cin in (('frames', 3), ('goal', 6)):
        images = rs.uniform(0, 1, (3, 2, H, W, cin)).astype(np.float32)
        got = scorer.embed(images, tower)
        assert got.shape == (3, 2, 24) and np.isfinite(got).all() and np.abs(got).max() > 0
        out[tower] = _digest(got)
    return out


def regnet_digest(H, W, m, ncam):
    """Digest of ``flow`` on 2 pairs."""
    from visual_foresight_amd.video_prediction.registration_net import HipRegistrationNet
    net = HipRegistrationNet('', dict(image_height=H, image_width=W, ncam=ncam, ch_mult=m, max_pairs=2, seed=11,
                                      bias_scale=0.1)).restore()
    rs = np.random.RandomState(2000 + H + W + m)
    cur, ref = (rs.uniform(0, 1, (2, ncam, H, W, 3)).astype(np.float32) for _ in range(2))
    got = net.flow(cur, ref)
    assert got.shape == (2, ncam, H, W, 2) and np.isfinite(got).all() and np.abs(got).max() > 0
    return _digest(got)


def _scorer_key(H, W, tower):
    return 'scorer %dx%d embedding 24 ncam 2 %s' % (H, W, tower)


def _regnet_key(H, W, m, ncam):
    return 'regnet %dx%d ch_mult %d ncam %d' % (H, W, m, ncam)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('H,W', SCORER_CASES)
def test_scorer_bits(H, W):
    want = _golden()
    for tower, got in scorer_digests(H, W).items():
        assert got == want[_scorer_key(H, W, tower)], 'the %s tower at %dx%d changed its bits' % (tower, H, W)


@pytest.mark.parametrize('H,W,m,ncam', REGNET_CASES)
def test_regnet_bits(H, W, m, ncam):
    assert regnet_digest(H, W, m, ncam) == _golden()[_regnet_key(H, W, m, ncam)], 'the flow changed its bits'


def mint(path):
    from visual_foresight_amd import _lib
    print('minting with %s' % _lib.LIB_PATH)
    out = {}
    for H, W in SCORER_CASES:
        for tower, d in scorer_digests(H, W).items():
            out[_scorer_key(H, W, tower)] = d
    for case in REGNET_CASES:
        out[_regnet_key(*case)] = regnet_digest(*case)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('minted %d digests into %s' % (len(out), path))


if __name__ == '__main__':
    if len(sys.argv) != 3 or sys.argv[1] != '--mint':
        sys.exit('usage: PYTHONPATH=<tree of the commit before the change> python %s --mint OUT.json' % sys.argv[0])
    mint(sys.argv[2])
