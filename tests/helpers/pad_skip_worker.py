"""Child process of tests/test_gpu_pad_skip.py: seeded rollouts of several shapes and plans, every output saved to an .npz.

The engine reads VF_PAD_SKIP once at creation, so the parent runs this worker once with VF_PAD_SKIP=0 (full K loops) and
once with the default (the gate-split tile skips kernel rows that read only padding) and compares the files bit for bit.
    python -m tests.helpers.pad_skip_worker OUT.npz
"""
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
from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config  # noqa: E402

# name, arch, H, W, T, samples, designated pixels, views, context frames
CASES = [
    ('c64_m200', 'cdna', 64, 64, 3, 200, 1, 1, 2),      # the flagship's tile plans (128-row gate-split tile)
    ('c64_m16', 'cdna', 64, 64, 3, 16, 1, 1, 2),        # small batch: the 32- / 64-row plans run too
    ('c48x64_m24', 'cdna', 48, 64, 3, 24, 2, 1, 2),     # 12 x 16 layers: row blocks below the image
    ('c48x64_m200', 'cdna', 48, 64, 2, 200, 1, 1, 2),
    ('c64_views2', 'cdna', 64, 64, 3, 20, 1, 2, 2),
    ('c64_ctx1', 'cdna', 64, 64, 3, 40, 1, 1, 1),       # one context frame (context de-duplication differs)
    ('savp_m24', 'savp', 64, 64, 3, 24, 1, 1, 2),       # arch 1
    ('savp2_m24', 'savp2', 64, 64, 3, 24, 1, 1, 2),     # arch 2: border-class bias epilogue
    ('savp3_m12', 'savp3', 64, 64, 3, 12, 1, 1, 2),     # arch 3: raw-gates variant of the same tile
]


def run(name, arch, H, W, T, M, nd, ncam, nc, seed, out):
    adim = 4 if arch == 'cdna' else (12 if arch == 'savp3' else 6)
    hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=adim, sdim=5, image_height=H, image_width=W,
              sequence_length=T + nc, n_context=nc, arch=arch, ncam=ncam)
    if arch == 'cdna':
        cfg = CdnaConfig(height=H, width=W, ndesig=nd, sequence_length=T + nc, n_context=nc)
        weights = [CdnaWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    elif arch == 'savp3':
        hp['zdim'] = 8
        cfg = Savp3Config(height=H, width=W, adim=adim, ndesig=nd, sequence_length=T + nc, zdim=8)
        weights = [SavpWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    else:
        cfg = (Savp2Config if arch == 'savp2' else SavpConfig)(height=H, width=W, adim=adim, ndesig=nd,
                                                               sequence_length=T + nc)
        weights = [SavpWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    pred = HipVPredEvaluation('', hp)
    pred.restore(weights if ncam > 1 else weights[0])
    rs = np.random.RandomState(seed)
    desig = rs.randint(0, min(H, W), (ncam, nd, 2))
    ctx = {'context_frames': rs.randint(0, 256, (nc, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (nc - 1, adim)), 'context_states': rs.normal(0, 0.1, (nc, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, nc, ncam, H, W, nd)}
    actions = rs.normal(0, 0.1, (M, T, adim))
    goal = rs.randint(0, min(H, W), (ncam, nd, 2))
    scores, per_task = pred.score(ctx, {'actions': actions}, goal)
    scores = np.asarray(scores)
    got = pred(ctx, {'actions': actions[:min(M, 8)]})
    out[name + '/scores'] = scores
    out[name + '/per_task'] = np.asarray(per_task)
    out[name + '/elites'] = np.argsort(scores, kind='stable')[:max(1, M // 10)]
    for k in sorted(got):
        out[name + '/' + k] = np.asarray(got[k])
    print('%-12s done' % name, flush=True)


def main():
    out = {}
    for i, case in enumerate(CASES):
        run(*case, seed=11 + i, out=out)
    np.savez(sys.argv[1], **out)


if __name__ == '__main__':
    main()
