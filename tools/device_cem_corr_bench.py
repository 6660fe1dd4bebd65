#!/usr/bin/env python
"""What the device-resident CEM route saves for the correlated-noise sampler: one ``PixelCostController`` planning call at
the shape of ``experiments/robonet/franka/franka.py`` (48 x 64, nactions 10, 5 CEM iterations, 20 elites, one designated
pixel, seeded random weights, ``verbose=False``) timed on the GPU, in one process, the variants alternating call by call and
rotating their order:

  correlated  ``CorrelatedNoiseSampler`` (np.random; elites by argsort on the host): the route such an experiment takes today
  host        ``PhiloxCorrelatedNoiseSampler`` with ``device_cem=False``: the float64 twin on the host
  device      ``PhiloxCorrelatedNoiseSampler`` on the device route: every iteration enqueued, one download

at 200 samples and at a 25-sample shard.  Host clock around ``act()``, which ends in a download on every route; median / min /
max over ``--calls`` calls after ``--warmup`` warm-ups.  Then the two kernels alone (``--launches`` back-to-back launches
between two events, so a figure includes the launch gap), and the kernels against the twin on the cases of
``tests/helpers/device_cem_corr_cases.py``: how many action values differ at all, the largest ``soft`` distance and the
largest centre error as a fraction of its bound.

    python tools/device_cem_corr_bench.py [--calls 15] [--warmup 3] [--out profiles/device_cem_correlated.txt]
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

H, W, NACTIONS, ITERATIONS, ELITES = 48, 64, 10, 5, 20
CONFIGS = (('200 samples', 200), ('25-sample shard', 25))
VARIANTS = ('correlated', 'host', 'device')


def make_controller(variant, num_samples):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.policy.cem_controllers.samplers import CorrelatedNoiseSampler, PhiloxCorrelatedNoiseSampler
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pol = dict(predictor_class=HipVPredEvaluation, verbose=False, nactions=NACTIONS, iterations=ITERATIONS,
               minimum_selection=ELITES, sampler=CorrelatedNoiseSampler)
    if num_samples != 200:          # (a policy dict may not restate a default)
        pol['num_samples'] = num_samples
    if variant != 'correlated':
        pol.update(sampler=PhiloxCorrelatedNoiseSampler, sampler_seed=1)
    if variant == 'host':
        pol['device_cem'] = False
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController({'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}, pol, 0, 1)
        ctrl.reset()
    return ctrl


def kernel_times(say, launches):
    """Each of the two kernels alone, at the two sizes."""
    import torch
    from tests.helpers import device_cem_corr_cases as cases
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceCorrelatedCEM
    for M in (200, 25):
        for refit_cov in (False, True):
            s = cases.make_sampler(4, nactions=NACTIONS, sampler_seed=1, refit_cov=refit_cov)
            dc = DeviceCorrelatedCEM(s, ELITES, 1, M, 'cuda:0')
            dc.upload()
            scores = torch.from_numpy(np.random.RandomState(M).normal(1.0, 0.5, M)).to(dc.device)
            cand = dc.sample(0, M, 0)
            dc.refit(0, scores, cand)
            ms = {}
            for what, launch in (('sample', lambda: dc.sample(0, M, 1)), ('soft refit', lambda: dc.refit(0, scores, cand))):
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
            say('  M %3d, refit_cov %-5s: cem_sample_corr_kernel %6.2f us, cem_soft_refit_kernel %6.2f us per launch'
                % (M, refit_cov, 1e3 * ms['sample'], 1e3 * ms['soft refit']))


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

    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    say('device-resident CEM, correlated noise: one PixelCostController planning call (%d iterations x (sample, rollout T%d, '
        'elites, soft refit)),' % (ITERATIONS, NACTIONS))
    say('%d x %d, %d elites, host clock around act(), %d calls after %d warm-ups, the three variants alternating in one process'
        % (H, W, ELITES, args.calls, args.warmup))
    for label, num_samples in CONFIGS:
        ctrls = {v: make_controller(v, num_samples) for v in VARIANTS}
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            for c in ctrls.values():
                c.act(t=0, i_tr=0, desig_pix=[[24, 32]], goal_pix=[[12, 48]], images=frames[:1], state=states[:1])
        times = {v: [] for v in VARIANTS}
        for i in range(args.warmup + args.calls):
            for v in VARIANTS[i % 3:] + VARIANTS[:i % 3]:
                c = ctrls[v]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    c.act(t=1, i_tr=0, desig_pix=[[24, 32]], goal_pix=[[12, 48]], images=frames, state=states)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    times[v].append(dt)
        assert type(ctrls['device']._device_cem).__name__ == 'DeviceCorrelatedCEM'
        assert getattr(ctrls['host'], '_device_cem', None) is None
        say('  %s:' % label)
        med = {}
        for v in VARIANTS:
            ms = np.asarray(times[v])
            med[v] = float(np.median(ms))
            say('    %-10s median %8.3f ms  (min %8.3f, max %8.3f)' % (v, med[v], ms.min(), ms.max()))
            assert ctrls[v].predictor.device_status() == 0
        say('    device route saves %.3f ms of the host route (%.1f %%) and %.3f ms of CorrelatedNoiseSampler (%.1f %%): %.3f ms '
            'per iteration' % (med['host'] - med['device'], 100 * (1 - med['device'] / med['host']),
                               med['correlated'] - med['device'], 100 * (1 - med['device'] / med['correlated']),
                               (med['correlated'] - med['device']) / ITERATIONS))
        del ctrls
    say('the two kernels alone (%d back-to-back launches between two events: a figure includes the launch gap):' % args.launches)
    kernel_times(say, args.launches)
    from tests.helpers import device_cem_corr_cases as cases
    say('kernels against the float64 twin (synthetic scores):')
    for name in sorted(cases.CASES):
        got, want = cases.device_run(name)
        adim = want['adim']
        pairs = [cases.action_excess(g[:, :, :adim], w[:, :, :adim]) for g, w in zip(got['calls'], want['calls'])]
        ulps = np.concatenate([u.reshape(-1) for _, u in pairs])
        inside = all(float(e.max()) <= 0.0 for e, _ in pairs)
        bound = cases.centre_bound(want['elite_rows'], want['soft'])
        err = np.abs(got['centre'] - want['centre'])
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        exact = np.array_equal(got['elites'], want['elites'])
        if 'fit_A' in want:
            exact = exact and np.array_equal(got['mean'], want['fit_mean']) and np.array_equal(got['A'], want['fit_A'])
        say('  %-11s M %3d K %3d: %d of %d action values differ at all (largest %d float32 ulp, inside the tolerance: %s); soft '
            'at most %d ulp; centre error at most %.4f of its bound; elites%s equal: %s'
            % (name, want['M'], want['K'], int((ulps > 0).sum()), ulps.size, int(ulps.max()), inside,
               int(cases.f64_ulp_distance(got['soft'], want['soft']).max()), frac,
               ', mean, A' if 'fit_A' in want else '', exact))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
