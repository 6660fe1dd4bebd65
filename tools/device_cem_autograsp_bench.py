#!/usr/bin/env python
"""What the device-resident CEM route saves for the autograsp sampler: milliseconds per planning call on one GPU,
``PixelCostController`` on a 64 x 64 CDNA engine with ``adim`` 5 (four moves and the gripper), nactions 5 x repeat 3, 3
iterations, default ``rejection_sampling``, at 200 samples and at a 25-sample shard.  Three routes alternate call by call in
one process and rotate their order (as ``tools/device_cem_frames_bench.py``):

    device     ``PhiloxAutograspSampler`` on the device route
    host       ``PhiloxAutograspSampler`` with ``device_cem=False``: the float64 twin on the host
    autograsp  ``AutograspSampler`` (np.random, one ``multivariate_normal`` call per rejected draw)

Host clock around ``act()``, which ends in a download on every route; median / min / max over ``--calls`` calls after
``--warmup`` warm-ups.  Then the kernels alone, and the kernels against the twin on the cases of
``tests/helpers/device_cem_autograsp_cases.py``: how many move values and how many gripper values differ.

    python tools/device_cem_autograsp_bench.py [--calls 15] [--warmup 3] [--out profiles/device_cem_autograsp.txt]
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

VARIANTS = ('device', 'host', 'autograsp')


def controller(variant, num_samples):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.policy.cem_controllers.samplers import AutograspSampler, PhiloxAutograspSampler
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pol = dict(predictor_class=HipVPredEvaluation, verbose=False, sampler=AutograspSampler)
    if num_samples != 200:
        pol['num_samples'] = num_samples
    if variant != 'autograsp':
        pol.update(sampler=PhiloxAutograspSampler, sampler_seed=1)
    if variant == 'host':
        pol['device_cem'] = False
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController({'adim': 5, 'sdim': 5, 'image_height': 64, 'image_width': 64}, pol, 0, 1)
        ctrl.reset()
    return ctrl


def kernel_time(say, launches):
    import torch
    from tests.helpers import device_cem_autograsp_cases as cases
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceAutograspCEM
    for M, K, no_refit in ((200, 10, True), (200, 10, False), (25, 10, True)):
        s = cases.make_sampler(5, sampler_seed=1, no_refit=no_refit)
        s.start_planning_call(np.array([0.9, 0.1, 0.25, 0., 0.]))
        with contextlib.redirect_stdout(io.StringIO()):
            mean, std = s.initial_proposal(0)
        dc = DeviceAutograspCEM(s, K, 2, M, 'cuda:0')
        dc.upload(mean, np.diag(std))
        scores = torch.from_numpy(np.random.RandomState(M).normal(1.0, 0.5, M)).to(dc.device)
        cand = dc.sample(0, M, 0)
        ms = {}
        after = 'after a refit (R = %d, %s)' % (K, 'by height' if no_refit else 'by share: two kernels')
        for what, launch in (('first proposal (R = 20, by height)', lambda: dc.sample(0, M, 1)),
                             ('refit', lambda: dc.refit(0, scores, cand)), (after, lambda: dc.sample(1, M, 2))):
            for _ in range(10):
                launch()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(launches):
                launch()
            stop.record()
            torch.cuda.synchronize()
            ms[what] = start.elapsed_time(stop) / launches
        say('  M %3d: ' % M + ', '.join('%s %.2f us' % (k, 1e3 * v) for k, v in ms.items()) + ' per launch')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('device-resident CEM, autograsp sampler: one planning call, host clock around act(), %d calls after %d warm-ups, '
        'the routes alternating in one process' % (args.calls, args.warmup))
    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (2, 1, 64, 64, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    states[:, 2] = 0.25                 # a height from which the plans end on either side of z_thresh
    kw = dict(desig_pix=[[32, 32]], goal_pix=[[16, 48]])
    for num_samples in (200, 25):
        ctrls = {v: controller(v, num_samples) for v in VARIANTS}
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            for c in ctrls.values():
                c.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
        times = {v: [] for v in VARIANTS}
        n = len(VARIANTS)
        for i in range(args.warmup + args.calls):
            for v in VARIANTS[i % n:] + VARIANTS[:i % n]:
                c = ctrls[v]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    c.act(t=1, i_tr=0, images=frames, state=states, **kw)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    times[v].append(dt)
        assert type(ctrls['device']._device_cem).__name__ == 'DeviceAutograspCEM'
        assert all(getattr(ctrls[v], '_device_cem', None) is None for v in VARIANTS[1:])
        say('  PixelCostController, %d samples, 64 x 64, adim 5, T15, 3 iterations, 10 elites:' % num_samples)
        med, spread = {}, {}
        for v in VARIANTS:
            ms = np.asarray(times[v])
            med[v], spread[v] = float(np.median(ms)), float(ms.max() - ms.min())
            say('    %-9s median %9.3f ms  (min %9.3f, max %9.3f)' % (v, med[v], ms.min(), ms.max()))
            assert ctrls[v].predictor.device_status() == 0
        say('    trials per sample of the device route\'s last call: mean %.1f, max %d; capped so far: %d'
            % (ctrls['device']._sampler.last_trials.mean(), ctrls['device']._sampler.last_trials.max(),
               ctrls['device']._sampler.n_capped))
        for v in VARIANTS[1:]:
            gain = med[v] - med['device']
            note = '' if abs(gain) > max(spread[v], spread['device']) else ' - no larger than the run-to-run spread'
            say('    the device route saves %.3f ms of %s (%.1f %%): %.3f ms per iteration%s'
                % (gain, v, 100 * (1 - med['device'] / med[v]), gain / 3, note))
        del ctrls
    say('the kernels alone (%d back-to-back launches between two events: a figure includes the launch gap; refit: '
        'cem_refit_kernel, the others cem_sample_autograsp_kernel, by share behind cem_grip_share_kernel):' % args.launches)
    kernel_time(say, args.launches)
    from tests.helpers import device_cem_autograsp_cases as cases
    say('cem_sample_autograsp_kernel / cem_grip_share_kernel / cem_refit_kernel against the float64 twin (a first proposal and '
        'two refits on synthetic scores):')
    moves_off = grip_off = 0
    for name in sorted(cases.CASES):
        got, want = cases.device_run(name)
        n = want['sampler']._adim
        ulps = np.concatenate([cases.ulp_distance(g[:, :, :n], w[:, :, :n].astype(np.float32)).reshape(-1)
                               for g, w in zip(got['calls'], want['calls'])])
        grip = sum(int((g[:, :, n] != w[:, :, n].astype(np.float32)).sum()) for g, w in zip(got['calls'], want['calls']))
        n_grip = sum(g[:, :, n].size for g in got['calls'])
        exact = all(np.array_equal(got[k][r], want[k][r]) for k in ('elites', 'fit_mean', 'fit_A') for r in range(2))
        moves_off += int((ulps > 0).sum())
        grip_off += grip
        say('  %-12s M %3d K %3d: %d of %d move values differ at all (largest %d float32 ulp), %d of %d gripper values; '
            'elites, mean, A equal: %s' % (name, want['M'], want['K'], int((ulps > 0).sum()), ulps.size, int(ulps.max()), grip,
                                           n_grip, exact))
    say('  over all cases %d move values and %d gripper values differ from the twin' % (moves_off, grip_off))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
