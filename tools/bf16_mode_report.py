#!/usr/bin/env python
"""GPU box: what the plain-bf16 precision mode (precision = 2) buys and what it costs, next to precisions 0 and 1.

    python tools/bf16_mode_report.py [--out FILE]    # all three blocks -> profiles/bf16_mode.txt

Three blocks, each measured by ONE process that interleaves the modes on one box (so box-to-box spread cancels); the driver
starts each block as a child under its own `timeout` and stops at the first one that fails:

  launch    rollout launch time (vf_get_profile: device time of the persistent launch) of precisions 0 / 1 / 2 at three
            sizes - C2 (200 x T13, 64x64), the 25-sample shard, and the C5 shard shape on arch 1 (625 sequences = 125 samples
            x 5 draws, T15, 128x128)
  accuracy  distance to the float64 oracle of frames, distributions and scores, the way tools/precision_check.py computes it
            (64x64, T13, 12 samples), plus the rounding twin of the oracle (tests/helpers/oracle_bf16.py) for scale
  elite     20 C2 planning calls (200 samples x T13, 3 CEM iterations, 10 elites) on the same seeds in precision 0 and in
            precision 2: elite overlap per iteration, whether the returned action is the same, rank correlation of the scores

No target is fixed for the elite agreement: it is the number a user decides on.
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'profiles', 'bf16_mode.txt')
MODES = ('fp32', 'bf16x6', 'bf16')
STEPS = (('launch', 420), ('accuracy', 300), ('elite', 420))        # block, time limit in seconds


def emit(line=''):
    print(line, flush=True)
    with open(OUT, 'a') as f:
        f.write(line + '\n')


def block_launch():
    import numpy as np
    import torch
    from oracle import pixel_cost
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    emit('== rollout launch time, ms (vf_get_profile; modes interleaved round by round in one process; median [min .. max])')
    sizes = (('C2: 200 x T13, 64x64, arch 0', 'cdna', 64, 200, 13, 4, 7),
             ('25-sample shard: 25 x T13, 64x64, arch 0', 'cdna', 64, 25, 13, 4, 11),
             ('C5 shard: 625 (125 x 5 draws) x T15, 128x128, arch 1', 'savp', 128, 625, 15, 12, 4))
    for name, arch, S, M, T, adim, rounds in sizes:
        rs = np.random.RandomState(5)
        ctx = {'context_frames': rs.randint(0, 256, (2, 1, S, S, 3)).astype(np.uint8),
               'context_actions': rs.normal(0, .05, (1, adim)), 'context_states': rs.normal(0, .1, (2, 5)),
               'context_pixel_distributions': pixel_cost.one_hot_distrib([[[S // 2, S // 2]]], 2, 1, S, S, 1)}
        acts = rs.normal(0, 0.05, (M, T, adim))
        goal = np.array([[[S // 4, 3 * S // 4]]])
        preds = {}
        for prec in MODES:
            hp = dict(designated_pixel_count=1, run_batch_size=M, adim=adim, sdim=5, image_height=S, image_width=S,
                      sequence_length=T + 2, precision=prec)
            if arch != 'cdna':
                hp['arch'] = arch
            preds[prec] = HipVPredEvaluation('', hp).restore()
            preds[prec].score(ctx, {'actions': acts}, goal)             # warm-up (schedule build, caches)
        times = {prec: [] for prec in MODES}
        for _ in range(rounds):
            for prec in MODES:
                p = preds[prec]
                p.set_profiling(True)
                p.score(ctx, {'actions': acts}, goal)
                torch.cuda.synchronize()
                ms, launches, _, _ = p.get_profile()
                p.set_profiling(False)
                times[prec].append(ms / max(launches, 1))
        emit(name)
        for prec in MODES:
            t = np.array(times[prec])
            emit('    %-7s %8.2f  [%.2f .. %.2f]  (%d launches)' % (prec, np.median(t), t.min(), t.max(), len(t)))
        m = {prec: float(np.median(times[prec])) for prec in MODES}
        emit('    bf16 / bf16x6 = %.3f   bf16 / fp32 = %.3f' % (m['bf16'] / m['bf16x6'], m['bf16'] / m['fp32']))
        del preds
    return 0


def block_accuracy():
    import numpy as np
    import torch
    from oracle import pixel_cost
    from oracle.cdna_predictor import OracleCdna
    from tests.helpers.oracle_bf16 import OracleCdnaBf16
    from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    H = W = 64
    T, M = 13, 12
    rs = np.random.RandomState(5)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8), 'context_actions': rs.normal(0, .05, (1, 4)),
           'context_states': rs.normal(0, .1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib([[[32, 32]]], 2, 1, H, W, 1)}
    acts = rs.normal(0, 0.05, (M, T, 4))
    goal = np.array([[[16, 48]]])
    weights = CdnaWeights.random(CdnaConfig(sequence_length=T + 2), seed=0)
    args = (ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'], ctx['context_states'], acts)
    f64, d64, _ = OracleCdna(weights, torch.float64).rollout(*args)
    want64, _ = pixel_cost.eval_pixel_cost(d64, goal, 10.)
    dmax = d64.max((3, 4), keepdims=True)

    def row(name, f, d, sc):
        emit('    %-28s frames max %.3g rms %.3g | distributions (rel. map max) max %.3g rms %.3g | scores rel max %.3g'
             % (name, np.abs(f - f64).max(), np.sqrt(np.mean((f - f64) ** 2)), (np.abs(d - d64) / dmax).max(),
                np.sqrt(np.mean(((d - d64) / dmax) ** 2)), np.abs(sc / want64 - 1).max()))
    emit('== distance to the float64 oracle (64x64, T13, %d samples, weights seed 0)' % M)
    f32, d32, _ = OracleCdna(weights, torch.float32).rollout(*args)
    row('CPU oracle, float32', f32, d32, pixel_cost.eval_pixel_cost(d32, goal, 10.)[0])
    ft, dt, _ = OracleCdnaBf16(weights, torch.float64).rollout(*args)
    row('rounding twin, float64', ft, dt, pixel_cost.eval_pixel_cost(dt, goal, 10.)[0])
    scores = {}
    for prec in MODES:
        pred = HipVPredEvaluation('', dict(designated_pixel_count=1, run_batch_size=M, sequence_length=T + 2,
                                           precision=prec)).restore(weights)
        sc, _ = pred.score(ctx, {'actions': acts}, goal)
        got = pred(ctx, {'actions': acts})
        scores[prec] = sc
        row('HIP ' + prec, got['predicted_frames'], got['predicted_pixel_distributions'], sc)
    for prec in MODES[1:]:
        emit('    score order identical, %s vs fp32: %s; vs float64 oracle: %s' % (
            prec, np.array_equal(scores['fp32'].argsort(), scores[prec].argsort()),
            np.array_equal(scores[prec].argsort(), want64.argsort())))
    emit('    min score gap %.3g   max |fp32 - bf16| %.3g' % (np.diff(np.sort(want64)).min(),
                                                           np.abs(scores['fp32'] - scores['bf16']).max()))
    return 0


def _rank_corr(a, b):
    import numpy as np
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])


def block_elite():
    import numpy as np
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    calls, K = 20, 10

    class HipBf16(HipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(HipBf16, self).__init__(model_path, dict(hparams, precision='bf16'), n_gpus, first_gpu)

    ag = {'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}
    base = {'nactions': 13, 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    ctrls = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for name, cls in (('fp32', HipVPredEvaluation), ('bf16', HipBf16)):
            ctrls[name] = PixelCostController(dict(ag), dict(base, predictor_class=cls), 0, 1)
    emit('== elite agreement, precision 2 against precision 0: %d C2 planning calls (200 samples x T13, 3 CEM iterations, %d '
         'elites), same seeds' % (calls, K))
    emit('   call  elite overlap itr0 itr1 itr2  same action  rank corr of scores itr0 (same candidates)')
    overlaps, same_action, corrs = [], 0, []
    for s in range(calls):
        frames = np.random.RandomState(100 + s).randint(0, 256, (2, 1, 64, 64, 3)).astype(np.uint8)
        states = np.random.RandomState(200 + s).normal(0, .1, (2, 5))
        rs = np.random.RandomState(300 + s)
        desig, goal = [[int(rs.randint(8, 56)), int(rs.randint(8, 56))]], [[int(rs.randint(8, 56)), int(rs.randint(8, 56))]]
        outs = {}
        for name in ('fp32', 'bf16'):
            with contextlib.redirect_stdout(io.StringIO()):
                c = ctrls[name]
                c.reset()
                np.random.seed(s)
                c.act(t=0, i_tr=0, desig_pix=desig, goal_pix=goal, images=frames[:1], state=states[:1])
                outs[name] = c.act(t=1, i_tr=0, desig_pix=desig, goal_pix=goal, images=frames, state=states)
        ov = []
        for itr in range(3):
            a, b = (np.argsort(outs[n]['plan_stat']['scores_itr%d' % itr], kind='stable')[:K] for n in ('fp32', 'bf16'))
            ov.append(len(set(a.tolist()) & set(b.tolist())))
        same = bool(np.array_equal(outs['fp32']['actions'], outs['bf16']['actions']))
        rc = _rank_corr(outs['fp32']['plan_stat']['scores_itr0'], outs['bf16']['plan_stat']['scores_itr0'])
        overlaps.append(ov); same_action += same; corrs.append(rc)
        emit('   %4d  %13d/%d %2d/%d %2d/%d  %-11s  %.6f' % (s, ov[0], K, ov[1], K, ov[2], K, same, rc))
    o = np.array(overlaps, np.float64)
    emit('   mean elite overlap per iteration: %.2f / %.2f / %.2f of %d (iterations 1 and 2 sample from the previous elites, so '
         'a differing elite set compounds); same returned action in %d of %d calls; rank correlation min %.6f median %.6f'
         % (o[:, 0].mean(), o[:, 1].mean(), o[:, 2].mean(), K, same_action, calls, min(corrs), float(np.median(corrs))))
    return 0


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument('--block', choices=[s for s, _ in STEPS])
    ap.add_argument('--out', default=OUT, help='report file (default profiles/bf16_mode.txt)')
    a = ap.parse_args()
    OUT = os.path.abspath(a.out)
    if a.block:
        return {'launch': block_launch, 'accuracy': block_accuracy, 'elite': block_elite}[a.block]()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('plain-bf16 precision mode (precision = 2) next to precisions 0 and 1: tools/bf16_mode_report.py, one box\n\n')
    for block, limit in STEPS:          # each GPU step under its own time limit; the first failure ends the report
        rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--block', block,
                              '--out', OUT])
        if rc != 0:
            emit('!! block %s ended with exit status %d: report stopped' % (block, rc))
            return rc
        emit()
    return 0


if __name__ == '__main__':
    sys.exit(main())
