#!/usr/bin/env python
"""Time area resampling on the GPU (profiles/resample.txt is this tool's output).

  (a) ``vf_resize_area`` alone at the shapes the controllers use - 2 x 480x640x3 uint8 -> 48x64 (a context of two frames),
      the same with two views (4 images), 3 x 192x256x3 float32 -> 96x128 (start, goal and one context frame of the
      inverse-model experiments) - with HIP events around BATCHES of back-to-back calls on one stream (a single call is a
      few microseconds: one event pair would time the event records), medians of ``--calls`` batches after ``--warmup``;
      against the bytes the call must move (source read once plus destination written) at the 6.3 TB/s streaming rate, and
      against what the same shrink costs without it: ``area_resize_host`` plus the upload of the small result, host clock
      around work that ends in a synchronise - on ONE thread (the function as it is: its NumPy loop is not threaded) and on
      16 threads (the images cut into bands of destination rows, one ``area_resize_host`` call per band in a pool of 16;
      exact for these integer ratios, and asserted equal).  The upload of the LARGE source, which the device path needs and
      the host path does not, is timed too.
  (b) one ``PixelCostController`` planning call (200 samples x T13, 3 CEM iterations - C2's counts - on a 48 x 64 model: C2's
      own 64 x 64 has another aspect ratio than a 480 x 640 camera, and the two must agree) fed 480 x 640 frames, against the
      same call of a second controller fed host-shrunk frames (the shrink itself outside its timed window, and reported),
      alternating in one process, every call with a new newest frame; host clock around ``act`` and the rollout launch time
      of ``vf_get_profile`` beside it, each with its spread.

(a) and (b) each run in a child process of their own under a time limit (``--step-timeout`` seconds): the parent never touches
the GPU, and a step that hangs or dies ends the run there, with nothing started after it.

    python tools/resample_bench.py [--calls 20] [--warmup 5] [--batch 200] [--planning-calls 9] [--step-timeout 300]
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

PEAK_GBS = 6300.0
SHAPES = [('context, 1 view', np.uint8, (2, 480, 640, 3), (48, 64)),
          ('context, 2 views', np.uint8, (2, 2, 480, 640, 3), (48, 64)),
          ('inverse model', np.float32, (3, 192, 256, 3), (96, 128))]


def med_spread(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


HOST_THREADS = 16


def host_shrink_threaded(x, size, pool):
    """``area_resize_host`` of ``x [..., Hs, Ws, C]`` at an INTEGER row ratio, cut into (image, band of destination rows)
    pieces for ``pool``: a band of destination rows reads exactly its own ``Hs / Hd`` source rows each, so the pieces are the
    whole result's."""
    from visual_foresight_amd.video_prediction.resample import area_resize_host
    Hs, Hd = x.shape[-3], size[0]
    assert Hs % Hd == 0
    f = Hs // Hd
    flat = x.reshape((-1,) + x.shape[-3:])
    bands = max(1, HOST_THREADS // flat.shape[0])
    edges = [Hd * b // bands for b in range(bands + 1)]
    jobs = [(i, lo, hi) for i in range(flat.shape[0]) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo]
    out = np.empty((flat.shape[0],) + tuple(size) + (x.shape[-1],), x.dtype)

    def one(job):
        i, lo, hi = job
        out[i, lo:hi] = area_resize_host(flat[i, lo * f:hi * f], (hi - lo, size[1]))
    list(pool.map(one, jobs))
    return out.reshape(x.shape[:-3] + out.shape[1:])


def time_kernel(calls, warmup, batch):
    import torch
    from visual_foresight_amd.video_prediction.resample import area_resize_device, area_resize_host
    torch.set_num_threads(min(HOST_THREADS, torch.get_num_threads()))
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    pool = ThreadPoolExecutor(HOST_THREADS)
    for name, dtype, shape, size in SHAPES:
        rs = np.random.RandomState(0)
        x = rs.randint(0, 256, shape).astype(np.uint8) if dtype == np.uint8 else rs.uniform(0, 1, shape).astype(np.float32)
        want = area_resize_host(x, size)
        d = torch.from_numpy(x).to(dev)
        assert np.array_equal(area_resize_device(d, size).cpu().numpy(), want), 'the timed call must reproduce the specification'
        us = []
        for i in range(warmup + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(batch):
                out = area_resize_device(d, size)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                us.append(1e3 * a.elapsed_time(b) / batch)
        del out
        med, lo, hi = med_spread(us)
        nbytes = x.nbytes + want.nbytes
        floor_us = nbytes / (PEAK_GBS * 1e3)
        print('(a) %-17s %s %s -> %dx%d: median %.2f us per call (min %.2f, max %.2f) over %d batches of %d back-to-back '
              'calls; moves %.3f MB = %.2f us at %.1f TB/s -> %.1f %% of the streaming rate'
              % (name, np.dtype(dtype).name, 'x'.join(map(str, shape)), size[0], size[1], med, lo, hi, calls, batch,
                 nbytes / 1e6, floor_us, PEAK_GBS / 1e3, 100 * floor_us / med))
        assert np.array_equal(host_shrink_threaded(x, size, pool), want), 'the banded host shrink must be the whole one'
        up, host, host16 = [], [], []
        for i in range(warmup + calls):
            t0 = time.perf_counter()
            torch.from_numpy(x).to(dev)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            small = area_resize_host(x, size)
            torch.from_numpy(small).to(dev)
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            small = host_shrink_threaded(x, size, pool)
            torch.from_numpy(small).to(dev)
            torch.cuda.synchronize(dev)
            t3 = time.perf_counter()
            if i >= warmup:
                up.append(1e3 * (t1 - t0))
                host.append(1e3 * (t2 - t1))
                host16.append(1e3 * (t3 - t2))
        print('    %-17s upload of the source %.3f ms (min %.3f, max %.3f); area_resize_host + upload of the result: one '
              'thread %.2f ms (min %.2f, max %.2f), %d threads %.2f ms (min %.2f, max %.2f); %d calls after %d'
              % ((name,) + med_spread(up) + med_spread(host) + (HOST_THREADS,) + med_spread(host16) + (calls, warmup)))
    pool.shutdown()


def time_planning(calls, warmup):
    import torch
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.resample import area_resize_host
    torch.set_num_threads(min(16, torch.get_num_threads()))
    Hc, Wc, H, W, T, M = 480, 640, 48, 64, 13, 200
    # (num_samples = 200 and iterations = 3 are the defaults, and a policy dict may not repeat a default)
    pol = {'nactions': T, 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    ags = {'camera 480x640': {'adim': 4, 'sdim': 5, 'image_height': Hc, 'image_width': Wc, 'model_image_height': H,
                              'model_image_width': W},
           'host-shrunk 48x64': {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}}
    rs = np.random.RandomState(1)
    pool = rs.randint(0, 256, (warmup + calls + 2, 1, Hc, Wc, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    kw = dict(desig_pix=[[24, 32]], goal_pix=[[12, 48]])
    with contextlib.redirect_stdout(io.StringIO()):
        ctrls = {name: PixelCostController(dict(ag), dict(pol), 0, 1) for name, ag in ags.items()}
        for name, c in ctrls.items():
            c.reset()
            c.predictor.set_profiling(True)
            first = pool[:1] if name.startswith('camera') else area_resize_host(pool[:1], (H, W))
            c.act(t=0, i_tr=0, images=first, state=states[:1], **kw)
            c.predictor.get_profile()
    wall = {name: [] for name in ctrls}
    kern = {name: [] for name in ctrls}
    shrink = []
    actions = {}
    for i in range(warmup + calls):
        frames = pool[i:i + 2]                  # a new newest frame every call: the context is uploaded (and shrunk) each time
        for name, c in ctrls.items():           # alternating: both see the same box at the same time
            if name.startswith('camera'):
                images = frames
            else:
                t0 = time.perf_counter()
                images = area_resize_host(frames, (H, W))
                shrink.append(1e3 * (time.perf_counter() - t0))
            np.random.seed(i)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out = c.act(t=1, i_tr=0, images=images, state=states, **kw)
            ms = 1e3 * (time.perf_counter() - t0)
            k = c.predictor.get_profile()[0]
            actions[name] = out['actions']
            if i >= warmup:
                wall[name].append(ms)
                kern[name].append(k)
        assert np.array_equal(actions['camera 480x640'], actions['host-shrunk 48x64']), 'both must plan the same action'
    for name in ctrls:
        med, lo, hi = med_spread(wall[name])
        kmed, klo, khi = med_spread(kern[name])
        print('(b) %-18s planning call (200 x T13 x 48x64, 3 iterations): act() median %.2f ms (min %.2f, max %.2f, spread '
              '%.2f %%); rollout launches %.3f ms (min %.3f, max %.3f, spread %.2f %%) over %d calls'
              % (name, med, lo, hi, 100 * (hi - lo) / med, kmed, klo, khi, 100 * (khi - klo) / kmed, calls))
    a, b = np.median(wall['camera 480x640']), np.median(wall['host-shrunk 48x64'])
    ka, kb = np.median(kern['camera 480x640']), np.median(kern['host-shrunk 48x64'])
    print('(b) camera / host-shrunk: act() %.4f (%+.2f %%), rollout launches %.4f (%+.2f %%); the host shrink the second '
          'controller\'s caller pays outside its act(): median %.2f ms (min %.2f, max %.2f); both planned the same actions'
          % ((a / b, 100 * (a / b - 1), ka / kb, 100 * (ka / kb - 1)) + med_spread(shrink)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=200)
    ap.add_argument('--planning-calls', type=int, default=9)
    ap.add_argument('--step-timeout', type=float, default=300.)
    ap.add_argument('--step', choices=('kernel', 'planning'), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is None:       # the parent: one fresh child per step, each under its own time limit; stop at the first failure
        for step in ('kernel', 'planning'):
            sys.stdout.flush()
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:],
                                    timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit('step %r did not finish in %.0f s; nothing further is started' % (step, args.step_timeout))
            if rc != 0:
                raise SystemExit('step %r ended with exit code %d; nothing further is started' % (step, rc))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench.py measures on a GPU; none is visible')
    if args.step == 'kernel':
        print('area resampling on %s' % torch.cuda.get_device_name(0))
        time_kernel(args.calls, args.warmup, args.batch)
    else:
        time_planning(args.planning_calls, 2)


if __name__ == '__main__':
    main()
