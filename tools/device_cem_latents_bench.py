#!/usr/bin/env python
"""What the device-resident CEM route saves for the latent-draw, ensemble and registration planners: milliseconds per
planning call on one GPU, the device route against the host route with the classes this project had before it
(``GaussianCEMSampler`` with ``StochasticHipPredictor`` / ``EnsembleHipPredictor`` / ``HipVPredEvaluation``), the two
alternating call by call in one process and swapping their order (as ``tools/device_cem_bench.py``).  Steps:

  c5        ``PixelCostController``, one rank's share of BASELINE C5: 125 actions x 5 latent draws, T15, 128 x 128, arch 1
            (device: ``PhiloxStochasticHipPredictor``)
  ensemble  ``CEM_Controller_Ensemble_Vidpred`` at C2 (200 samples, T13, 64 x 64) with E = 4 members
  c3        ``RegisterGtruthController`` at C3 (2 views x 600 samples, T13, 64 x 64, start + goal registration, 30 elites)
  kernels   ``cem_latents_kernel`` + ``cem_fold_latents_kernel`` per launch at the C5 share's shape, from a
            ``rocprofv3 --kernel-trace --stats`` run of its own (a fresh child process)
  ulps      the kernels against ``philox_latents`` / ``fold_latents`` on the shapes of
            ``tests/test_gpu_device_cem_latents.py``: how many latent values differ at all

Host clock around ``act()``, which ends in a download on every route; median / min / max over ``--calls`` calls after
``--warmup`` warm-ups.  Both routes run the samplers' default ``rejection_sampling``: at ``repeat`` 1 and 13 - 15 actions the
parent's figure is then mostly ``GaussianCEMSampler``'s rejection loop on the host.

    python tools/device_cem_latents_bench.py [--step c5,ensemble,c3,kernels,ulps] [--calls 5] [--warmup 1]
                                             [--out profiles/device_cem_latents.txt]
"""
import argparse
import contextlib
import csv
import glob
import io
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

C5_SHAPE = (5, 15, 8, 125, 4)       # n_latent, T, zdim, actions, width


def _policy(variant, **over):
    from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxGaussianCEMSampler
    pol = dict(verbose=False, repeat=1, **over)
    if variant == 'device':
        pol.update(sampler=PhiloxGaussianCEMSampler, sampler_seed=1)
    return pol


def c5_controller(variant):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.stochastic_predictor import PhiloxStochasticHipPredictor, StochasticHipPredictor
    cls = PhiloxStochasticHipPredictor if variant == 'device' else StochasticHipPredictor
    pol = _policy(variant, predictor_class=cls.with_options(n_latent=5, arch='savp'), nactions=15, num_samples=125,
                  vpred_batch_size=125)
    return PixelCostController({'adim': 4, 'sdim': 5, 'image_height': 128, 'image_width': 128}, pol, 0, 1)


def ensemble_controller(variant):
    from visual_foresight_amd.policy.cem_controllers.variants.ensemble_vidpred import CEM_Controller_Ensemble_Vidpred
    pol = _policy(variant, nactions=13)
    return CEM_Controller_Ensemble_Vidpred({'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}, pol, 0, 1)


def c3_controller(variant):
    from bench import smooth_flow_warper
    from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController
    pol = _policy(variant, nactions=13, num_samples=600, vpred_batch_size=600, designated_pixel_count=2, selection_frac=0.05,
                  registration_warper=smooth_flow_warper, register_region=True, trade_off_reg=True)
    return RegisterGtruthController({'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64, 'ncam': 2}, pol, 0, 1)


# step -> (label, size, views, tasks per view, constructor, whether act() takes a goal image)
COMPARISONS = {
    'c5': ('PixelCostController, one rank\'s C5 share: 125 actions x 5 latent draws, T15, 128 x 128, arch 1, 3 iterations',
           128, 1, 1, c5_controller, False),
    'ensemble': ('CEM_Controller_Ensemble_Vidpred at C2: 200 samples, T13, 64 x 64, E = 4, 3 iterations', 64, 1, 1,
                 ensemble_controller, False),
    'c3': ('RegisterGtruthController at C3: 2 views x 600 samples, T13, 64 x 64, start + goal registration with the trade-off, '
           '30 elites, 3 iterations', 64, 2, 1, c3_controller, True),
}
VARIANTS = ('device', 'parent')


def step_compare(step, say, calls, warmup):
    import torch
    label, size, ncam, ntask, make, wants_goal = COMPARISONS[step]
    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (2, ncam, size, size, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    k = size // 64
    kw = dict(desig_pix=[[k * (32 - 3 * i), k * (32 + 2 * i)] for i in range(ncam * ntask)],
              goal_pix=[[k * (16 + 2 * i), k * (48 - 3 * i)] for i in range(ncam * ntask)])
    if wants_goal:
        kw['goal_image'] = rs.uniform(0, 1, (1, ncam, size, size, 3)).astype(np.float32)
    ctrls = {}
    np.random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        for v in VARIANTS:
            ctrls[v] = make(v)
            ctrls[v].reset()
            ctrls[v].act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
    times = {v: [] for v in VARIANTS}
    for i in range(warmup + calls):
        for v in VARIANTS[i % 2:] + VARIANTS[:i % 2]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                ctrls[v].act(t=1, i_tr=0, images=frames, state=states, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                times[v].append(dt)
    assert type(ctrls['device']._device_cem).__name__ == 'DeviceCEM'
    assert getattr(ctrls['parent'], '_device_cem', None) is None
    say('  %s:' % label)
    med = {}
    for v in VARIANTS:
        ms = np.asarray(times[v])
        med[v] = float(np.median(ms))
        say('    %-7s median %9.3f ms  (min %9.3f, max %9.3f) over %d calls' % (v, med[v], ms.min(), ms.max(), len(ms)))
        assert ctrls[v].predictor.device_status() == 0
    say('    the device route saves %.3f ms of the parent\'s host route (%.2f %%): %.3f ms per iteration'
        % (med['parent'] - med['device'], 100 * (1 - med['device'] / med['parent']), (med['parent'] - med['device']) / 3))


def _draw_and_fold(nl, T, zdim, M, width, seed, call, actions=None):
    import torch
    from visual_foresight_amd import _lib
    lib = _lib.load_library()
    if actions is None:
        actions = torch.zeros((M, T, width), dtype=torch.float32, device='cuda:0')
    z = torch.empty((nl, T, zdim), dtype=torch.float32, device='cuda:0')
    seqs = torch.empty((M * nl, T, width + zdim), dtype=torch.float32, device='cuda:0')
    _lib.check(lib.vf_cem_latents(0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, call & 0xFFFFFFFF, nl, T, zdim,
                                  z.data_ptr(), None))
    _lib.check(lib.vf_cem_fold_latents(0, actions.data_ptr(), z.data_ptr(), M, nl, T, width, zdim, seqs.data_ptr(), None))
    return z, seqs


def step_kernels_child(launches):
    import torch
    nl, T, zdim, M, width = C5_SHAPE
    for call in range(launches):
        _draw_and_fold(nl, T, zdim, M, width, 1, call)
    torch.cuda.synchronize()


def step_kernels(say, launches):
    """One ``rocprofv3 --kernel-trace --stats`` run (kernel tracing only, no counters) of a fresh child process."""
    rocprof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    tmp = tempfile.mkdtemp(prefix='vf_latents_prof_')
    try:
        cmd = [rocprof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable,
               os.path.abspath(__file__), '--step', 'kernels-child', '--launches', str(launches)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=REPO)
        if proc.returncode:
            print(proc.stdout[-3000:])
            raise SystemExit(proc.returncode)
        traces = glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True)
        if not traces:
            raise SystemExit('rocprofv3 wrote no kernel trace under %s' % tmp)
        per = {}
        with open(traces[0]) as f:
            for row in csv.DictReader(f):
                name = row['Kernel_Name'].split('(')[0]
                if 'cem_latents_kernel' in name or 'cem_fold_latents_kernel' in name:
                    per.setdefault(name, []).append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
        say('  draw + fold at the C5 share\'s shape (n_latent %d, T %d, zdim %d, %d actions of width %d), per launch, from one '
            'rocprofv3 --kernel-trace --stats run:' % C5_SHAPE)
        total = 0.0
        for name, ns in sorted(per.items()):
            total += float(np.median(ns))
            say('    %-52s median %7.2f us  (min %7.2f, max %7.2f) over %d launches'
                % (name[-52:], np.median(ns) / 1e3, min(ns) / 1e3, max(ns) / 1e3, len(ns)))
        say('    both: %.2f us per scoring call' % (total / 1e3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_ulps(say):
    import torch
    from tests.helpers.device_cem_cases import ulp_distance
    from visual_foresight_amd.video_prediction.stochastic_predictor import fold_latents, philox_latents
    say('  cem_latents_kernel / cem_fold_latents_kernel against philox_latents / fold_latents (three (seed, call) pairs a shape):')
    all_differing = all_total = largest = 0
    for nl, T, zdim, M, width in [(1, 1, 1, 1, 1), (2, 3, 3, 5, 4), (5, 15, 8, 9, 5), (3, 13, 16, 4, 4), (2, 20, 16, 3, 4), C5_SHAPE]:
        actions = np.random.RandomState(T).normal(0, 0.1, (M, T, width)).astype(np.float32)
        differing = total = 0
        folds = True
        for seed, call in [(31, 0), (31, 2 ** 32 - 1), ((0x01234567 << 32) | 0x89ABCDEF, 5)]:
            z, seqs = _draw_and_fold(nl, T, zdim, M, width, seed, call, torch.from_numpy(actions).to('cuda:0'))
            got = z.cpu().numpy()
            ulps = ulp_distance(got, philox_latents(seed, call, nl, T, zdim).astype(np.float32))
            differing, total, largest = differing + int((ulps > 0).sum()), total + ulps.size, max(largest, int(ulps.max()))
            folds = folds and seqs.cpu().numpy().tobytes() == fold_latents(actions, got).tobytes()
        say('    n_latent %d, T %2d, zdim %2d, M %3d, width %d: %d of %d latent values differ at all; the fold bit for bit: %s'
            % (nl, T, zdim, M, width, differing, total, folds))
        all_differing, all_total = all_differing + differing, all_total + total
    say('    %d of %d latent values differ from the specification, the largest distance %d float32 ulp'
        % (all_differing, all_total, largest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', default='c5,ensemble,c3,kernels,ulps')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if args.step == 'kernels-child':
        return step_kernels_child(args.launches)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    steps = args.step.split(',')
    if any(s in COMPARISONS for s in steps):
        say('device-resident CEM, latent-draw / ensemble / registration planners: one planning call, host clock around act(), '
            '%d calls after %d warm-ups, device route and parent host route alternating in one process' % (args.calls, args.warmup))
    for step in steps:
        if step in COMPARISONS:
            step_compare(step, say, args.calls, args.warmup)
        elif step == 'kernels':
            step_kernels(say, args.launches)
        elif step == 'ulps':
            step_ulps(say)
        else:
            raise SystemExit('unknown step %r' % step)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
