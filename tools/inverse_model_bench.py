#!/usr/bin/env python
"""Time the action-inference network of the inverse-model policy on the GPU (profiles/inverse_model.txt is this tool's
output).

Every step runs in a child process of its own under a time limit; the first step that fails ends the run.  Medians of 20
calls after 5 warm-ups:

  infer64 / infer96 / infer64x8   ``infer_device`` of one problem at 64x64 and at 96x128 and of eight problems at 64x64
                    (n_context 2, n_actions 15, adim 4), HIP events around the call on its stream, inputs resident on the
                    device; in the same run ``HostActionInference`` at 16 threads on the same problems plus the upload of
                    its actions (host clock around work that ends in a synchronise); the device's and the float32
                    restatement's error against the float64 restatement
  slope             the recurrence kernel's time per step: (time at n_actions 30 - time at n_actions 5) / 25 with the same
                    weights, 64x64, one problem - everything but the recurrence is the same in the two calls
  kernels           the per-kernel split of the three configurations from one ``rocprofv3 --kernel-trace --stats`` run
  act               a closed loop of ``InvModelBaseController.act`` (64x64, replan_every 1: every timed step plans) on the
                    device network and on the host network, host clock around ``act``

    python tools/inverse_model_bench.py [--calls 20] [--warmup 5] [--out profiles/inverse_model.txt]
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

STEPS = (('infer64', 300), ('infer96', 300), ('infer64x8', 300), ('slope', 300), ('kernels', 420), ('act', 300))
CONFIGS = {'infer64': (64, 64, 1), 'infer96': (96, 128, 1), 'infer64x8': (64, 64, 8)}     # H, W, n


def med_spread(ms):
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def make_nets(H, W, n, n_actions=15, weights=None):
    from visual_foresight_amd.video_prediction.inverse_model import HipActionInference, HostActionInference
    hp = dict(image_height=H, image_width=W, adim=4, n_context=2, n_actions=n_actions, max_batch=n, seed=11, bias_scale=0.1)
    dev = HipActionInference(weights if weights is not None else '', hp).restore()
    return dev, HostActionInference(dev.weights, hp).restore()


def problems(n, H, W, adim=4, nc=2):
    rs = np.random.RandomState(0)
    img = (H, W, 3)
    return (rs.uniform(0, 1, (n,) + img).astype(np.float32), rs.uniform(0, 1, (n,) + img).astype(np.float32),
            rs.uniform(-1, 1, (n, nc, adim)).astype(np.float32), rs.uniform(0, 1, (n, nc) + img).astype(np.float32))


def device_ms(dev, d_inputs, calls, warmup):
    import torch
    stream = torch.cuda.current_stream(dev.device)
    ms = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = dev.infer_device(*d_inputs)
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms, out


def step_infer(name, calls, warmup):
    import torch
    from tests.helpers import oracle_inverse_model as ora
    H, W, n = CONFIGS[name]
    dev, host = make_nets(H, W, n)
    inputs = problems(n, H, W)
    d_inputs = tuple(torch.from_numpy(a).to(dev.device) for a in inputs)
    ms, out = device_ms(dev, d_inputs, calls, warmup)
    med, lo, hi = med_spread(ms)
    print('%-9s infer_device of %d problem(s) (%dx%d, n_context 2, n_actions 15, adim 4): median %.3f ms (min %.3f, max %.3f) over '
          '%d calls, six launches' % (name, n, H, W, med, lo, hi, calls))
    parts = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        actions = host.infer(*inputs)
        t1 = time.perf_counter()
        up = torch.from_numpy(actions).to(dev.device)
        torch.cuda.synchronize(dev.device)
        t2 = time.perf_counter()
        if i >= warmup:
            parts.append((t1 - t0, t2 - t1, t2 - t0))
    h = np.median(np.array(parts), axis=0) * 1e3
    print('%-9s HostActionInference (float32, %d threads) on the same problem(s): %.2f ms + upload of its %d actions %.3f ms = '
          'median %.2f ms over %d calls' % (name, torch.get_num_threads(), h[0], up.shape[0] * up.shape[1], h[1], h[2], calls))
    print('%-9s device %.3f ms against host twin + upload %.2f ms: the device path is %s (%.1f x)'
          % (name, med, h[2], 'faster' if med < h[2] else 'NOT faster', h[2] / med))
    a64, _ = ora.forward(dev.weights, *inputs, dtype=torch.float64)
    a32, _ = ora.forward(dev.weights, *inputs, dtype=torch.float32)
    a32b, _ = ora.forward(dev.weights, *inputs, dtype=torch.float32, order=1)
    got = out.cpu().numpy()
    print('%-9s actions against the float64 restatement (max abs error, largest |action| %.3g): device %.3g, float32 restatement '
          '%.3g (gate terms summed the other way round: %.3g); bound of the test: 8 x the restatement\'s = %.3g'
          % (name, np.abs(a64).max(), np.abs(got - a64).max(), np.abs(a32 - a64).max(), np.abs(a32b - a64).max(),
             8 * np.abs(a32 - a64).max()))


def step_slope(calls, warmup):
    import torch
    from visual_foresight_amd.video_prediction.inverse_model_arch import InverseModelConfig, InverseModelWeights
    H, W = 64, 64
    long_net, _ = make_nets(H, W, 1, n_actions=30)
    short_w = InverseModelWeights(InverseModelConfig(H, W, 4, 2, 5), long_net.weights.tensors)
    short_net, _ = make_nets(H, W, 1, n_actions=5, weights=short_w)
    d_inputs = tuple(torch.from_numpy(a).to(long_net.device) for a in problems(1, H, W))
    t30 = med_spread(device_ms(long_net, d_inputs, calls, warmup)[0])[0]
    t5 = med_spread(device_ms(short_net, d_inputs, calls, warmup)[0])[0]
    print('slope     infer_device at n_actions 30: median %.3f ms; at n_actions 5 with the same weights: %.3f ms -> '
          '%.2f us per step of the recurrence' % (t30, t5, 1e3 * (t30 - t5) / 25))


def step_kernels_child(calls, warmup):
    import torch
    for name in ('infer64', 'infer96', 'infer64x8'):
        H, W, n = CONFIGS[name]
        dev, _ = make_nets(H, W, n)
        d_inputs = tuple(torch.from_numpy(a).to(dev.device) for a in problems(n, H, W))
        for _ in range(warmup + calls):
            dev.infer_device(*d_inputs)
        torch.cuda.synchronize(dev.device)


def step_kernels(calls, warmup):
    """One ``rocprofv3 --kernel-trace --stats`` run of the three configurations (kernel tracing only, no counters)."""
    rocprof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    tmp = tempfile.mkdtemp(prefix='vf_invmodel_prof_')
    try:
        cmd = [rocprof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable,
               os.path.abspath(__file__), '--step', 'kernels-child', '--calls', str(calls), '--warmup', str(warmup)]
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
                kname = row['Kernel_Name']
                if 'invmodel' not in kname:
                    continue
                grid = (int(row.get('Grid_Size_X', 0) or 0), int(row.get('Workgroup_Size_X', 0) or 0))
                per.setdefault((kname.split('(')[0], grid), []).append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
        print('kernels   per launch, from one rocprofv3 --kernel-trace --stats run (%d + %d calls of each configuration; grid '
              'sizes tell the configurations apart: threads x workgroup size)' % (warmup, calls))
        for (kname, grid), ns in sorted(per.items(), key=lambda kv: (kv[0][0], kv[0][1])):
            print('kernels   %-44s grid %7d x %4d: median %8.2f us over %d launches'
                  % (kname[-44:], grid[0], grid[1], float(np.median(ns)) / 1e3, len(ns)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_act(calls, warmup):
    from visual_foresight_amd.policy.inverse_models import InvModelBaseController
    from visual_foresight_amd.video_prediction.inverse_model import HipActionInference, HostActionInference
    H = W = 64
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    rs = np.random.RandomState(1)
    steps = 2 + warmup + calls
    frames = rs.randint(0, 256, (steps, 1, H, W, 3)).astype(np.uint8)
    goal = rs.uniform(0, 1, (1, 1, H, W, 3))
    for label, cls in (('HipActionInference', HipActionInference), ('HostActionInference', HostActionInference)):
        ms = []
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = InvModelBaseController(dict(ag), {'predictor_class': cls, 'replan_every': 1}, 0, 1)
            ctrl.reset()
            np.random.seed(0)
            for t in range(steps):
                t0 = time.perf_counter()
                ctrl.act(t=t, i_tr=0, images=frames[max(0, t - 1):t + 1], goal_image=goal)
                if t >= 2 + warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
        med, lo, hi = med_spread(ms)
        print('act       InvModelBaseController.act (64x64, T 15, plans at every step, uint8 frame in, action out) with %-19s: '
              'median %.3f ms (min %.3f, max %.3f) over %d steps' % (label, med, lo, hi, calls))


def run_step(name, calls, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('inverse_model_bench.py measures on a GPU; none is visible')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if name in CONFIGS:
        step_infer(name, calls, warmup)
    elif name == 'slope':
        step_slope(calls, warmup)
    elif name == 'kernels':
        step_kernels(calls, warmup)
    elif name == 'kernels-child':
        step_kernels_child(calls, warmup)
    else:
        step_act(calls, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'inverse_model.txt'))
    ap.add_argument('--step', choices=[s for s, _ in STEPS] + ['kernels-child'],
                    help='run one step in this process (what the driver starts)')
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args.calls, args.warmup)
    lines = ['action-inference network of the inverse-model policy, medians of %d calls after %d warm-ups '
             '(tools/inverse_model_bench.py)' % (args.calls, args.warmup)]
    rc = 0
    for name, limit in STEPS:
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', name, '--calls',
               str(args.calls), '--warmup', str(args.warmup)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=REPO)
        print(proc.stdout, end='')
        sys.stdout.flush()
        if proc.returncode:
            lines.append('step %s FAILED with exit status %d; nothing further was started' % (name, proc.returncode))
            lines.extend(proc.stdout.splitlines()[-15:])
            rc = proc.returncode
            break
        lines.extend(proc.stdout.splitlines())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
