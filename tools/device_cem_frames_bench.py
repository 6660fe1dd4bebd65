#!/usr/bin/env python
"""What the device-resident CEM route saves for the frame-cost planners: milliseconds per planning call on one GPU, the
device route against host routes this project had before it, the variants alternating call by call in one process and
rotating their order (as ``tools/device_cem_bench.py``):

  goal image  ``GoalImController`` at 200 samples, 64 x 64, nactions 5 x repeat 3, 3 iterations:
                device    ``PhiloxGaussianCEMSampler`` on the device route
                gaussian  ``GaussianCEMSampler`` (np.random, rejection loop and np.cov on the host)
  towel       ``ClassifierController`` at the towel experiment's shape (18 x T15 at 48 x 64, appearance flow, a frames-only
              engine, 10 elites):
                device    ``PhiloxFoldingCEMSampler`` on the device route
                folding   ``FoldingCEMSampler`` (np.random)
                host      ``PhiloxFoldingCEMSampler`` with ``device_cem=False``: the float64 twin on the host

Host clock around ``act()``, which ends in a download on every route; median / min / max over ``--calls`` calls after
``--warmup`` warm-ups.  Then ``cem_sample_fold_kernel`` alone, and the kernel against the twin on the cases of
``tests/helpers/device_cem_fold_cases.py``: how many action values differ at all and the largest ulp distance.

    python tools/device_cem_frames_bench.py [--calls 15] [--warmup 3] [--out profiles/device_cem_frames.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

TOWEL_STATE_APPEND = [0.41, 0.25, 0.166]


def goal_controller(variant):
    from visual_foresight_amd.policy.cem_controllers import GoalImController
    from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxGaussianCEMSampler
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pol = dict(predictor_class=HipVPredEvaluation, verbose=False)
    if variant == 'device':
        pol.update(sampler=PhiloxGaussianCEMSampler, sampler_seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = GoalImController({'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}, pol, 0, 1)
        ctrl.reset()
    return ctrl


def towel_controller(variant):
    from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxFoldingCEMSampler
    from visual_foresight_amd.policy.cem_controllers.samplers.folding_sampler import FoldingCEMSampler
    from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController
    from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation

    class Flow(FramesOnlyHipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(Flow, self).__init__(model_path, dict(hparams, transformation='flow'), n_gpus, first_gpu)

    pol = dict(predictor_class=Flow, verbose=False, num_samples=18, selection_frac=0.05, initial_std=0.005,
               initial_std_lift=0.05, state_append=TOWEL_STATE_APPEND, sampler=FoldingCEMSampler)
    if variant != 'folding':
        pol.update(sampler=PhiloxFoldingCEMSampler, sampler_seed=1)
    if variant == 'host':
        pol['device_cem'] = False
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = ClassifierController({'adim': 4, 'sdim': 5, 'image_height': 48, 'image_width': 64}, pol, 0, 1)
        ctrl.reset()
    return ctrl


# label, (H, W), variants (the device route first), constructor, act() keywords given (frames, goal)
COMPARISONS = (
    ('GoalImController, 200 samples, 64 x 64, T15, 3 iterations, 10 elites', (64, 64), ('device', 'gaussian'), goal_controller,
     lambda goal: {'goal_image': goal}),
    ('ClassifierController, the towel shape: 18 samples, 48 x 64, T15, appearance flow, frames-only, 3 iterations, 10 elites',
     (48, 64), ('device', 'folding', 'host'), towel_controller, lambda goal: {}),
)
DRIVERS = {goal_controller: 'DeviceCEM', towel_controller: 'DeviceFoldingCEM'}


def fold_kernel_time(say, launches):
    import torch
    from tests.helpers import device_cem_fold_cases as cases
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceFoldingCEM
    for M, K in ((18, 10), (198, 10)):
        s = cases.make_sampler(sampler_seed=1, **cases.TOWEL_STD)
        mean, std = s.initial_proposal(1, np.array(cases.STATE))
        dc = DeviceFoldingCEM(s, K, 1, M, 'cuda:0')
        dc.upload(mean, np.diag(std))
        scores = torch.from_numpy(np.random.RandomState(M).normal(1.0, 0.5, M)).to(dc.device)
        cand = dc.sample(0, M, 0)
        ms = {}
        for what, launch in (('first proposal (R = 20)', lambda: dc.sample(0, M, 1)), ('refit', lambda: dc.refit(0, scores, cand)),
                             ('after a refit (R = %d)' % K, lambda: dc.sample(0, M, 2))):
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
        say('  M %3d: ' % M + ', '.join('%s %.2f us' % (k, 1e3 * v) for k, v in ms.items()) + ' per launch '
            '(refit: cem_refit_kernel, the others cem_sample_fold_kernel)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    warnings.simplefilter('ignore', RuntimeWarning)     # (FoldingCEMSampler's refitted covariance is singular, as the reference's)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('device-resident CEM, frame-cost planners: one planning call, host clock around act(), %d calls after %d warm-ups, '
        'the variants alternating in one process' % (args.calls, args.warmup))
    for label, (H, W), variants, make, act_kw in COMPARISONS:
        rs = np.random.RandomState(0)
        frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
        states = rs.uniform(0, 1, (2, 5))
        kw = act_kw(rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32))
        ctrls = {v: make(v) for v in variants}
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            for c in ctrls.values():
                c.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
        times = {v: [] for v in variants}
        n = len(variants)
        for i in range(args.warmup + args.calls):
            for v in variants[i % n:] + variants[:i % n]:
                c = ctrls[v]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    c.act(t=1, i_tr=0, images=frames, state=states, **kw)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    times[v].append(dt)
        assert type(ctrls['device']._device_cem).__name__ == DRIVERS[make]
        assert all(getattr(ctrls[v], '_device_cem', None) is None for v in variants[1:])
        say('  %s:' % label)
        med = {}
        for v in variants:
            ms = np.asarray(times[v])
            med[v] = float(np.median(ms))
            say('    %-9s median %8.3f ms  (min %8.3f, max %8.3f)' % (v, med[v], ms.min(), ms.max()))
            assert ctrls[v].predictor.device_status() == 0
        for v in variants[1:]:
            say('    the device route saves %.3f ms of %s (%.1f %%): %.3f ms per iteration'
                % (med[v] - med['device'], v, 100 * (1 - med['device'] / med[v]), (med[v] - med['device']) / 3))
        del ctrls
    say('the folding kernels alone (%d back-to-back launches between two events: a figure includes the launch gap):'
        % args.launches)
    fold_kernel_time(say, args.launches)
    from tests.helpers import device_cem_fold_cases as cases
    say('cem_sample_fold_kernel / cem_refit_kernel against the float64 twin (a first proposal and two refits on synthetic scores):')
    largest = 0
    for name in sorted(cases.CASES):
        got, want = cases.device_run(name)
        pairs = [cases.action_excess(g[:, :, :4], w[:, :, :4]) for g, w in zip(got['calls'], want['calls'])]
        ulps = np.concatenate([u.reshape(-1) for _, u in pairs])
        inside = all(float(e.max()) <= 0.0 for e, _ in pairs)
        exact = all(np.array_equal(got[k][r], want[k][r]) for k in ('elites', 'fit_mean', 'fit_A') for r in range(2))
        largest = max(largest, int(ulps.max()))
        say('  %-12s M %3d K %3d: %d of %d action values differ at all (largest %d float32 ulp, inside the tolerance: %s); '
            'elites, mean, A equal: %s' % (name, want['M'], want['K'], int((ulps > 0).sum()), ulps.size, int(ulps.max()), inside,
                                           exact))
    say('  largest distance of an action value from the twin over all cases: %d float32 ulp' % largest)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
