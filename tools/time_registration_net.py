#!/usr/bin/env python
"""Time the registration network on the GPU (profiles/registration_net.txt is this tool's output).

Every step runs in a child process of its own under a time limit; the first step that fails ends the run.  Medians of 20
calls after 5 warm-ups:

  flow64 / flow96   ``flow_device`` of 4 pairs (max_pairs = 2, ncam = 2) at 64x64 and at 96x128 with ch_mult = 4, HIP events
                    around the call on its stream, inputs resident on the device; the FLOPs the kernels execute (idle MFMA
                    rows and padded channel tiles included) and their share of the 157.3 TFLOP/s fp32 MFMA peak; in the
                    same run ``HostRegistrationNet`` at 16 threads on the same pairs plus the upload of its flow (host
                    clock around work that ends in a synchronise); the device's and the float32 restatement's error
                    against the float64 restatement
  accuracy          those two errors for every case of tests/test_gpu_registration_net.py
  planning          a C3 ``RegisterGtruthController`` planning call (600 samples x T13, two views, 64x64, 3 iterations) with
                    the device net as its warper against the same call with ``bench.smooth_flow_warper``, which has no
                    network at all; alternating in one process, host clock around ``act``

    python tools/time_registration_net.py [--calls 20] [--warmup 5] [--out profiles/registration_net.txt]
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

PEAK_TFLOPS = 157.3
STEPS = (('flow64', 300), ('flow96', 420), ('accuracy', 420), ('planning', 420))       # (name, time limit in seconds)
SHAPES = {'flow64': (64, 64), 'flow96': (96, 128)}


def executed_flops(cfg):
    """FLOPs the kernels execute per (pair, view): d1 and the flow head on the vector ALU (every tap counted), the five MFMA
    layers as whole 32-position tiles times whole 32-channel tiles, the up-sampling as four multiply-adds per output."""
    valu = mfma = 0
    for name, k, cin, cout, h, w in cfg.layers():
        if name in ('d1', 'flow'):
            valu += 2 * h * w * k * k * cin * cout
            continue
        tw = 16 if (name in ('d2', 'd3') or w % 16 == 0) else 8
        th = 32 // tw
        tiles = -(-w // tw) * -(-h // th)
        mfma += 2 * tiles * 32 * 9 * cin * (-(-cout // 32) * 32)
        if name.startswith('u'):
            valu += 2 * 4 * (2 * h) * (2 * w) * cout
    return valu, mfma


def med_spread(ms):
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def make_net(H, W, m=4, ncam=2, max_pairs=2):
    from visual_foresight_amd.video_prediction.registration_net import HipRegistrationNet, HostRegistrationNet
    hp = dict(image_height=H, image_width=W, ncam=ncam, ch_mult=m, max_pairs=max_pairs, seed=11, bias_scale=0.1)
    dev = HipRegistrationNet('', hp).restore()
    return dev, HostRegistrationNet(dev.weights, hp).restore()


def errors(weights, cur, ref, got):
    import torch
    from tests.helpers import oracle_registration_net as ora
    f64 = ora.forward_views(weights, cur, ref, torch.float64)
    f32 = ora.forward_views(weights, cur, ref, torch.float32)
    top = np.abs(f64).max()
    return np.abs(got - f64).max() / top, np.abs(f32 - f64).max() / top, top


def step_flow(name, calls, warmup):
    import torch
    H, W = SHAPES[name]
    dev, host = make_net(H, W)
    rs = np.random.RandomState(0)
    cur, ref = (rs.uniform(0, 1, (2, 2, H, W, 3)).astype(np.float32) for _ in range(2))
    d_cur, d_ref = (torch.from_numpy(a).to(dev.device) for a in (cur, ref))
    stream = torch.cuda.current_stream(dev.device)
    ms = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = dev.flow_device(d_cur, d_ref)
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    med, lo, hi = med_spread(ms)
    got = out.cpu().numpy()
    valu, mfma = executed_flops(dev.cfg)
    algo = 2 * sum(dev.cfg.macs_per_pair().values())
    tf = 4 * (valu + mfma) / med / 1e9
    print('%-8s flow_device of 4 pairs (2 x 2 views, %dx%d, ch_mult 4): median %.3f ms (min %.3f, max %.3f) over %d calls; '
          'executed %.2f GFLOP (%.2f MFMA + %.2f VALU; algorithmic %.2f) -> %.1f TFLOP/s = %.1f %% of %.1f'
          % (name, H, W, med, lo, hi, calls, 4 * (valu + mfma) / 1e9, 4 * mfma / 1e9, 4 * valu / 1e9, 4 * algo / 1e9, tf,
             100 * tf / PEAK_TFLOPS, PEAK_TFLOPS))
    parts = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        flow = host.flow(cur, ref)
        t1 = time.perf_counter()
        up = torch.from_numpy(flow).to(dev.device)
        torch.cuda.synchronize(dev.device)
        t2 = time.perf_counter()
        if i >= warmup:
            parts.append((t1 - t0, t2 - t1, t2 - t0))
    h = np.median(np.array(parts), axis=0) * 1e3
    print('%-8s HostRegistrationNet (float32, %d threads) on the same 4 pairs: %.2f ms + upload of its %.2f MB flow %.3f ms = '
          'median %.2f ms over %d calls' % (name, torch.get_num_threads(), h[0], up.numel() * 4 / 1e6, h[1], h[2], calls))
    print('%-8s condition: flow_device %.3f ms < host net + upload %.2f ms: %s (%.0f x)'
          % (name, med, h[2], 'MET' if med < h[2] else 'NOT MET', h[2] / med))
    e_dev, e_32, top = errors(dev.weights, cur, ref, got)
    print('%-8s flow against the float64 restatement (max abs error / largest |flow| %.2f px): device %.3g, float32 '
          'restatement %.3g; bound of the test: 8 x the latter = %.3g' % (name, top, e_dev, e_32, 8 * e_32))


def step_accuracy():
    from tests.test_gpu_registration_net import test_flow_against_the_float64_restatement as t
    cases = [m for m in t.pytestmark if m.name == 'parametrize'][0].args[1]
    for H, W, m, ncam, n in cases:
        dev, _ = make_net(H, W, m, ncam)
        rs = np.random.RandomState(H + W + m)
        cur, ref = (rs.uniform(0, 1, (n, ncam, H, W, 3)).astype(np.float32) for _ in range(2))
        e_dev, e_32, top = errors(dev.weights, cur, ref, dev.flow(cur, ref))
        print('accuracy %3dx%-3d ch_mult %d ncam %d n %d: device %.3g, float32 restatement %.3g of the largest |flow| %.2f px '
              '(ratio %.2f, allowed 8)' % (H, W, m, ncam, n, e_dev, e_32, top, e_dev / e_32))
        del dev


def step_planning(calls, warmup):
    import bench
    from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController
    M, T, iters, ncam, ndesig, size = bench.WORKLOADS['c3'][:6]
    dev, _ = make_net(size, size)
    ag = {'adim': 4, 'sdim': 5, 'image_height': size, 'image_width': size, 'ncam': ncam}
    pol = {'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'register_region': True, 'vpred_batch_size': M,
           'designated_pixel_count': ndesig, 'nactions': T, 'num_samples': M}
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, ncam, size, size, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    kw = dict(goal_image=rs.uniform(0, 1, (1, ncam, size, size, 3)).astype(np.float32), i_tr=0,
              desig_pix=[[32, 32], [29, 34]], goal_pix=[[16, 48], [18, 45]])
    warpers = {'device net': dev, 'smooth_flow_warper': bench.smooth_flow_warper}
    ctrls = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for name, w in warpers.items():
            ctrls[name] = RegisterGtruthController(dict(ag), dict(pol, registration_warper=w), 0, 1)
            ctrls[name].reset()
            ctrls[name].act(t=0, images=frames[:1], state=states[:1], **kw)
    ms = {name: [] for name in ctrls}
    np.random.seed(0)
    for i in range(warmup + calls):
        for name, c in ctrls.items():           # alternating: both see the same box at the same time
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                c.act(t=1, images=frames, state=states, **kw)
            if i >= warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    stats = {name: med_spread(v) for name, v in ms.items()}
    for name, (med, lo, hi) in stats.items():
        print('planning C3 RegisterGtruthController (%d x T%d x %d views x %dx%d, %d iterations) with %-18s: median %.2f ms '
              '(min %.2f, max %.2f) over %d calls' % (M, T, ncam, size, size, iters, name, med, lo, hi, calls))
    print('planning device net - smooth_flow_warper = %.2f ms per planning call'
          % (stats['device net'][0] - stats['smooth_flow_warper'][0]))


def run_step(name, calls, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_registration_net.py measures on a GPU; none is visible')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if name in SHAPES:
        step_flow(name, calls, warmup)
    elif name == 'accuracy':
        step_accuracy()
    else:
        step_planning(calls, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'registration_net.txt'))
    ap.add_argument('--step', choices=[s for s, _ in STEPS], help='run one step in this process (what the driver starts)')
    args = ap.parse_args()
    if args.step:
        return run_step(args.step, args.calls, args.warmup)
    lines = ['registration network, medians of %d calls after %d warm-ups (tools/time_registration_net.py)'
             % (args.calls, args.warmup)]
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
