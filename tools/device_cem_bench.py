#!/usr/bin/env python
"""What the device-resident CEM route saves: one ``PixelCostController`` planning call (3 CEM iterations, horizon
5 actions x 3 repeats, 64 x 64, one designated pixel, seeded random weights) timed on the GPU, in one process, the variants
alternating call by call and rotating their order:

  gaussian   ``GaussianCEMSampler`` (np.random, np.cov, per-sample multivariate_normal; elites by argsort on the host)
  host       ``PhiloxGaussianCEMSampler`` with ``device_cem=False``: the float64 twin on the host, scores downloaded per iteration
  device     ``PhiloxGaussianCEMSampler`` on the device route: every iteration enqueued, one download

at 200 samples fp32, 200 samples plain bf16 and the 25-sample shard (fp32), with the default ``rejection_sampling`` and
without it (the setting bench.py plans with).  Host clock around ``act()``, which ends in a
download on every route; median / min / max over ``--calls`` calls after ``--warmup`` warm-ups.  It also runs the kernels of
``csrc/vf_cem.h`` against the twin on the cases of ``tests/helpers/device_cem_cases.py`` and records how many action values
differ at all (they may differ by one float32 ulp: the device's float64 log / sin / cos).

    python tools/device_cem_bench.py [--calls 15] [--warmup 3] [--out profiles/device_cem.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

H = W = 64
CONFIGS = (('200 samples, fp32', 200, 'fp32', {}), ('200 samples, plain bf16', 200, 'bf16', {}),
           ('25-sample shard, fp32', 25, 'fp32', {}),
           # bench.py's planner setting: no rejection loop, one multivariate_normal call per iteration on the host
           ('200 samples, fp32, rejection_sampling False', 200, 'fp32', {'rejection_sampling': False}),
           ('25-sample shard, fp32, rejection_sampling False', 25, 'fp32', {'rejection_sampling': False}))
VARIANTS = ('gaussian', 'host', 'device')


def make_controller(variant, num_samples, precision, extra):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxGaussianCEMSampler
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pol = dict(extra, predictor_class=HipVPredEvaluation, verbose=False)
    if num_samples != 200:
        pol['num_samples'] = num_samples
    if variant != 'gaussian':
        pol.update(sampler=PhiloxGaussianCEMSampler, sampler_seed=1)
    if variant == 'host':
        pol['device_cem'] = False
    before = os.environ.get('VF_PRECISION')
    os.environ['VF_PRECISION'] = precision
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = PixelCostController({'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}, pol, 0, 1)
            ctrl.reset()
    finally:
        if before is None:
            del os.environ['VF_PRECISION']
        else:
            os.environ['VF_PRECISION'] = before
    return ctrl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    say('device-resident CEM: one PixelCostController planning call (3 iterations x (sample, rollout T15, elites, refit)),')
    say('%d x %d, host clock around act(), %d calls after %d warm-ups, the three variants alternating in one process' %
        (H, W, args.calls, args.warmup))
    for label, num_samples, precision, extra in CONFIGS:
        ctrls = {v: make_controller(v, num_samples, precision, extra) for v in VARIANTS}
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            for c in ctrls.values():
                c.act(t=0, i_tr=0, desig_pix=[[32, 32]], goal_pix=[[16, 48]], images=frames[:1], state=states[:1])
        times = {v: [] for v in VARIANTS}
        for i in range(args.warmup + args.calls):
            for v in VARIANTS[i % 3:] + VARIANTS[:i % 3]:
                c = ctrls[v]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    c.act(t=1, i_tr=0, desig_pix=[[32, 32]], goal_pix=[[16, 48]], images=frames, state=states)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    times[v].append(dt)
        say('  %s:' % label)
        med = {}
        for v in VARIANTS:
            ms = np.asarray(times[v])
            med[v] = float(np.median(ms))
            say('    %-9s median %8.3f ms  (min %8.3f, max %8.3f)' % (v, med[v], ms.min(), ms.max()))
            assert ctrls[v].predictor.device_status() == 0
        say('    device route saves %.3f ms of the host route (%.1f %%) and %.3f ms of the gaussian baseline (%.1f %%); capped '
            'samples: %d' % (med['host'] - med['device'], 100 * (1 - med['device'] / med['host']),
                             med['gaussian'] - med['device'], 100 * (1 - med['device'] / med['gaussian']),
                             ctrls['device']._sampler.n_capped))
        del ctrls
    from tests.helpers import device_cem_cases as cases
    say('kernels against the float64 twin (synthetic scores; elites, trials, capped flags, mean and A are equal):')
    for name in sorted(cases.CASES):
        got, want = cases.device_run(name)
        ulps = np.concatenate([cases.ulp_distance(g['actions'], w['actions'].astype(np.float32)).reshape(-1)
                               for g, w in zip(got['calls'], want['calls'])])
        exact = (np.array_equal(got['fit_mean'], want['fit_mean']) and np.array_equal(got['fit_A'], want['fit_A'])
                 and np.array_equal(got['elites'], want['elites']))
        say('  %-12s M %3d K %3d: %d of %d action values differ (largest distance %d ulp); mean, A, elites equal: %s'
            % (name, want['M'], want['K'], int((ulps > 0).sum()), ulps.size, int(ulps.max()), exact))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
