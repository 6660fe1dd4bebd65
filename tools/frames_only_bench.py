"""What does the distribution channel cost?  Frames-only engines (``designated_pixel_count`` 0) against the
same engines with one designated pixel - the behaviour before frames-only engines existed - on one GPU, one build, one process.

Per shape both engines are built from the same weights and roll the same sequences.  After a warm-up the two are timed
ALTERNATELY: ``--repeats`` (5) rounds, each 20 ``vf_rollout`` launches of one engine between two events on the launch stream,
then 20 of the other, the order swapped every round.  Reported per shape: the median over the rounds of the per-launch time of
each engine, the ratio of the medians, the spread (min .. max over the rounds) of each, the device bytes ``vf_create``
allocates (``hipMemGetInfo`` around it) and, for the planning shapes, one ``ClassifierController`` planning call with
either predictor class.  Writes ``profiles/frames_only.txt`` (``--out``).

    python tools/frames_only_bench.py [--out profiles/frames_only.txt] [--repeats 5] [--launches 20] [--quick]
"""
import argparse
import contextlib
import ctypes
import io
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name, predictor hyper-parameters, sequences per launch, horizon, plan with a ClassifierController?
SHAPES = [
    ('C2 200 x T13 64x64 cdna fp32', dict(image_height=64, image_width=64), 200, 13, True),
    ('C2 200 x T13 64x64 cdna bf16', dict(image_height=64, image_width=64, precision='bf16'), 200, 13, False),
    ('towel 18 x T13 48x64 flow', dict(image_height=48, image_width=64, transformation='flow'), 18, 13, True),
    ('towel 200 x T13 48x64 flow', dict(image_height=48, image_width=64, transformation='flow'), 200, 13, True),
    ('C5 shard 125 x 5 draws x T15 128x128 arch 1', dict(image_height=128, image_width=128, arch='savp', adim=12, n_draws=5),
     625, 15, False),
]


def build(hp, B, T, nd, weights=None):
    import torch
    from visual_foresight_amd.video_prediction.cdna_arch import CdnaWeights
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(dict(adim=4, sdim=5), **hp)
    draws = hp.get('n_draws', 1)
    free0 = torch.cuda.mem_get_info(0)[0]
    pred = HipVPredEvaluation('', dict(hp, designated_pixel_count=nd, run_batch_size=B // draws, sequence_length=T + 2))
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info(0)[0]
    if weights is None:
        weights = CdnaWeights.random(pred.cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)
    pred.restore(weights)
    return pred, weights, used


def launcher(pred, B, T, rs_seed=1):
    """-> a function that enqueues one vf_rollout of B sequences on the current stream."""
    import torch
    from visual_foresight_amd import _lib
    c = pred.cfg
    rs = np.random.RandomState(rs_seed)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, c.height, c.width, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, c.adim)), 'context_states': rs.normal(0, 0.1, (2, c.sdim))}
    if not pred.frames_only:
        d = np.zeros((2, 1, c.height, c.width, c.ndesig), np.float32)
        d[:, :, c.height // 2, c.width // 2] = 1.
        ctx['context_pixel_distributions'] = d
    pred._set_context(ctx)
    acts = torch.from_numpy(rs.normal(0, 0.1, (B, T, c.adim)).astype(np.float32)).to(pred.device)
    n = B // pred.n_draws
    scores = torch.empty(n, dtype=torch.float64, device=pred.device)
    per_task = torch.empty((n, max(c.ndesig, 1)), dtype=torch.float64, device=pred.device)
    goal = np.tile(np.array([c.height // 4, c.width // 4], np.int32), (1, max(c.ndesig, 1), 1))

    def launch():
        pred._rollout_chunk(acts, goal, 10., scores, per_task)
    return launch


def time_launches(launch, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def plan_call(predictor_class, hp, M, T):
    """Wall time of one ClassifierController planning call (3 CEM iterations) after one warm-up call."""
    import torch
    from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController

    class Selected(predictor_class):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            extra = {k: v for k, v in hp.items() if k in ('transformation', 'precision')}
            super(Selected, self).__init__(model_path, dict(hparams, **extra), n_gpus, first_gpu)

    H, W = hp['image_height'], hp['image_width']
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    pol = {'nactions': T, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'predictor_class': Selected}
    if M != 200:            # (an override equal to the default is refused, as in the reference)
        pol['num_samples'] = M
    rs = np.random.RandomState(2)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = ClassifierController(ag, pol, 0, 1)
        ctrl.reset()
        np.random.seed(0)
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1])
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ctrl.act(t=1, i_tr=0, images=frames, state=states)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
    assert ctrl.predictor.device_status() == 0
    return min(times[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'frames_only.txt'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--quick', action='store_true', help='two small shapes: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    import torch
    from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation, HipVPredEvaluation
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    shapes = SHAPES if not a.quick else [('quick 8 x T3 32x32 cdna', dict(image_height=32, image_width=32), 8, 3, True),
                                         ('quick 8 x T3 48x64 flow', dict(image_height=48, image_width=64, transformation='flow'), 8, 3, False)]
    lines = ['frames-only engines against the same engines with one designated pixel (tools/frames_only_bench.py)',
             'device: %s; %d rounds of %d launches per engine, alternating, after 3 warm-up launches each'
             % (torch.cuda.get_device_name(0), a.repeats, a.launches),
             'times in ms per vf_rollout launch (events on the launch stream); bytes: hipMemGetInfo around vf_create', '']
    # (the first engine of a process also pays for loading the code object: spend that on a small one, outside the byte counts)
    warm = build(dict(image_height=32, image_width=32), 1, 3, 1)[0]
    for name, hp, B, T, plan in shapes:
        p1, w, bytes1 = build(hp, B, T, 1)
        p0, _, bytes0 = build(hp, B, T, 0, w)
        l0, l1 = launcher(p0, B, T), launcher(p1, B, T)
        for l in (l0, l1):
            time_launches(l, 3)
        t0s, t1s = [], []
        for r in range(a.repeats):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (t0s if which == 0 else t1s).append(time_launches(l0 if which == 0 else l1, a.launches))
        assert p0.device_status() == 0 and p1.device_status() == 0
        m0, m1 = float(np.median(t0s)), float(np.median(t1s))
        lines += ['%s' % name,
                  '  one designated pixel : median %8.3f  rounds %s  spread %.3f' % (m1, ' '.join('%.3f' % t for t in t1s), max(t1s) - min(t1s)),
                  '  frames-only          : median %8.3f  rounds %s  spread %.3f' % (m0, ' '.join('%.3f' % t for t in t0s), max(t0s) - min(t0s)),
                  '  frames-only / one pixel = %.4f  (difference %.3f ms; spread of the one-pixel rounds %.3f ms)'
                  % (m0 / m1, m0 - m1, max(t1s) - min(t1s)),
                  '  device bytes of vf_create: one pixel %d, frames-only %d, saved %d (%.1f MB)'
                  % (bytes1, bytes0, bytes1 - bytes0, (bytes1 - bytes0) / 1e6)]
        del p0, p1, l0, l1
        if plan:
            ms1, out1 = plan_call(HipVPredEvaluation, hp, B, T)
            ms0, out0 = plan_call(FramesOnlyHipVPredEvaluation, hp, B, T)
            same = all(np.array_equal(out0['plan_stat'][k], out1['plan_stat'][k]) for k in out1['plan_stat'] if k.startswith('scores'))
            lines.append('  ClassifierController planning call (3 iterations, best of 2 after a warm-up): HipVPredEvaluation %.1f ms, '
                         'FramesOnlyHipVPredEvaluation %.1f ms; scores of every iteration %s'
                         % (ms1, ms0, 'identical' if same else 'DIFFER'))
        lines.append('')
        print('\n'.join(lines[-(7 if plan else 6):]), flush=True)
    del warm
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
