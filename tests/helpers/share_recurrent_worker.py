"""Child process of tests/test_gpu_share_recurrent.py: seeded planning calls of several shapes, batch sizes, context lengths,
architectures and both launch strategies, every output saved to an .npz.

The engine reads VF_SHARE_RECURRENT once at creation, so the parent runs this worker once with VF_SHARE_RECURRENT=0 (every
sample computes the recurrent gate sums on the still shared h(s-1) itself) and once with the default (one shared partial,
the per-sample items start from it) and compares the files bit for bit - except the `meta/` entries, the MFMA FLOPs the
engine's profile counts as executed for the first rollout of each case, which tell the parent where the partial ran.
    python -m tests.helpers.share_recurrent_worker OUT.npz
"""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from oracle import pixel_cost  # noqa: E402  (one_hot_distrib only: input construction)
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights  # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation  # noqa: E402
from visual_foresight_amd.video_prediction.savp_arch import Savp2Config, SavpConfig  # noqa: E402
from visual_foresight_amd.video_prediction.savp_arch import CdnaWeights as SavpWeights  # noqa: E402

# name, arch, H, W, T, samples, designated pixels, views, context frames, persistent launch
CASES = [
    ('c64_m1', 'cdna', 64, 64, 3, 1, 1, 1, 2, 1),
    ('c64_m3', 'cdna', 64, 64, 3, 3, 1, 1, 2, 1),
    ('c64_m25', 'cdna', 64, 64, 3, 25, 1, 1, 2, 1),
    ('c64_m200', 'cdna', 64, 64, 3, 200, 1, 1, 2, 1),           # the flagship's tile plans
    ('c48x64_m1', 'cdna', 48, 64, 3, 1, 1, 1, 2, 1),            # 6 x 8 / 12 x 16 / 24 x 32 layers: tiles past the image
    ('c48x64_m3', 'cdna', 48, 64, 3, 3, 2, 1, 2, 1),
    ('c48x64_m25', 'cdna', 48, 64, 3, 25, 1, 1, 2, 1),
    ('c48x64_m200', 'cdna', 48, 64, 2, 200, 1, 1, 2, 1),
    ('c64_ctx1', 'cdna', 64, 64, 3, 25, 1, 1, 1, 1),            # one context frame: nothing is emitted (lstm1-4 would qualify
    ('c64_ctx1_m200', 'cdna', 64, 64, 2, 200, 1, 1, 1, 1),      # at step 1 - at these batches their plans could consume it)
    ('c64_ctx3_m25', 'cdna', 64, 64, 3, 25, 1, 1, 3, 1),        # three: an all-shared step in front of the partial's
    ('c64_ctx3_m200', 'cdna', 64, 64, 2, 200, 1, 1, 3, 1),
    ('c64_views2', 'cdna', 64, 64, 3, 20, 1, 2, 2, 1),
    ('c64_m25_layers', 'cdna', 64, 64, 3, 25, 1, 1, 2, 0),      # one launch per layer
    ('c64_m200_layers', 'cdna', 64, 64, 2, 200, 1, 1, 2, 0),
    ('c48x64_ctx3_layers', 'cdna', 48, 64, 3, 3, 1, 1, 3, 0),
    ('savp_m24', 'savp', 64, 64, 3, 24, 1, 1, 2, 1),            # arch 1
    ('savp_m100', 'savp', 64, 64, 2, 100, 1, 1, 2, 1),
    ('savp2_m24', 'savp2', 64, 64, 3, 24, 1, 1, 2, 1),          # arch 2: all seven conv-LSTMs, border-class bias epilogue
    ('savp2_m100', 'savp2', 64, 64, 2, 100, 1, 1, 2, 1),
    ('savp2_m24_layers', 'savp2', 64, 64, 2, 24, 1, 1, 2, 0),
    ('savp_128_m125', 'savp', 128, 128, 2, 125, 1, 1, 2, 1),    # the 64 x 64 core at a batch that takes the 128-row plans
    ('savp2_128_m125', 'savp2', 128, 128, 2, 125, 1, 1, 2, 1),
]


def _context(rs, nc, ncam, H, W, nd, adim):
    desig = rs.randint(0, min(H, W), (ncam, nd, 2))
    return {'context_frames': rs.randint(0, 256, (nc, ncam, H, W, 3)).astype(np.uint8),
            'context_actions': rs.normal(0, 0.05, (max(nc - 1, 0), adim)), 'context_states': rs.normal(0, 0.1, (nc, 5)),
            'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, nc, ncam, H, W, nd)}


def _keep(out, key, arr):
    """Small arrays as they are; large ones (the frames of 200 samples) as the digest of their bytes."""
    arr = np.ascontiguousarray(arr)
    if arr.nbytes <= (8 << 20):
        out[key] = arr
    else:
        out[key + '/sha256'] = np.frombuffer(hashlib.sha256(arr.tobytes()).digest(), dtype=np.uint8)


def run(name, arch, H, W, T, M, nd, ncam, nc, persistent, seed, out):
    adim = 4 if arch == 'cdna' else 6
    hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=adim, sdim=5, image_height=H, image_width=W,
              sequence_length=T + nc, n_context=nc, arch=arch, ncam=ncam, persistent=persistent)
    if arch == 'cdna':
        cfg = CdnaConfig(height=H, width=W, ndesig=nd, sequence_length=T + nc, n_context=nc)
        weights = [CdnaWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    else:
        cfg = (Savp2Config if arch == 'savp2' else SavpConfig)(height=H, width=W, adim=adim, ndesig=nd,
                                                               sequence_length=T + nc)
        weights = [SavpWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    pred = HipVPredEvaluation('', hp)
    pred.restore(weights if ncam > 1 else weights[0])
    rs = np.random.RandomState(seed)
    goal = rs.randint(0, min(H, W), (ncam, nd, 2))
    # one planning call = several rollouts on one context (the first computes the shared units, the later ones reuse
    # them), then a changed context (recomputed), then the first context again
    ctx_a, ctx_b = _context(rs, nc, ncam, H, W, nd, adim), _context(rs, nc, ncam, H, W, nd, adim)
    for tag, ctx, rollouts in (('a', ctx_a, 3), ('b', ctx_b, 2), ('a2', ctx_a, 1)):
        for it in range(rollouts):
            actions = rs.normal(0, 0.1, (M, T, adim))
            first = tag == 'a' and it == 0
            if first:
                pred.set_profiling(True)
            scores, per_task = pred.score(ctx, {'actions': actions}, goal)
            if first:       # executed FLOPs of the rollout that computes the shared units (per layer: of its conv-LSTM kernels)
                out['meta/%s/flops' % name] = np.float64(pred.get_profile()[2])
                pred.set_profiling(False)
            key = '%s/%s%d' % (name, tag, it)
            out[key + '/scores'] = np.asarray(scores)
            out[key + '/per_task'] = np.asarray(per_task)
        got = pred(ctx, {'actions': actions})      # frames, distributions and states of every sample of the last rollout
        for k in sorted(got):
            _keep(out, '%s/%s/%s' % (name, tag, k), np.asarray(got[k]))
    print('%-20s done' % name, flush=True)


def main():
    out = {}
    for i, case in enumerate(CASES):
        run(*case, seed=23 + i, out=out)
    np.savez(sys.argv[1], **out)


if __name__ == '__main__':
    main()
