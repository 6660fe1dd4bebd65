#!/usr/bin/env python
"""Time the plan visualisation on the GPU (profiles/plan_render_cost.txt is this tool's output).

At C2 (200 sequences x T13 x 64x64, cdna, one designated pixel) with the K = 10 best plans it reports, as medians of 20
calls after 5 warm-ups:

  (a) ``vf_render_plans`` alone on the resident rollout: HIP events around the call on the rollout's stream, with the
      bytes it reads and writes;
  (b) ``HipVPredEvaluation.render_plans`` host clock around the whole call (upload of the indices and the table, the
      kernels, the device-to-host copy of the bytes) - resident, and re-rolled (the ten plans rolled again as one batch);
  (c) the same page's bytes without the entry point: ``__call__`` (every one of the 200 videos exported and copied to
      the host), pick ten, colour them in NumPy (``visualizer/colormap.py``);
  (d) one planning call (3 CEM iterations) of ``PixelCostController`` with ``verbose=True`` and a worker that discards
      its messages against the same call with ``verbose=False``, alternating in the same process, host clock around
      ``act``.

    python tools/time_plan_render.py [--calls 20] [--warmup 5]
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
T, M, K = 13, 200, 10


def med_spread(ms):
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def line(tag, what, ms, calls, extra=''):
    med, lo, hi = med_spread(ms)
    print('c2 K=%d (%s) %-58s median %.4f ms (min %.4f, max %.4f) over %d calls%s' % (K, tag, what, med, lo, hi, calls, extra))


def time_render(calls, warmup):
    import torch
    from visual_foresight_amd import _lib
    from visual_foresight_amd.policy.cem_controllers.visualizer import colormap
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=1, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2)
    pred = HipVPredEvaluation('', hp).restore()
    rs = np.random.RandomState(0)
    distrib = np.zeros((2, 1, H, W, 1), np.float32)
    distrib[:, :, H // 2, W // 2] = 1.
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': distrib}
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = [[[16, 48]]]
    scores = pred.score(ctx, {'actions': actions}, goal_pix=goal)[0]
    best = scores.argsort()[:K]
    want = pred.render_plans(best)
    read = K * T * H * W * (3 + 2 * 1) * 4          # frames once, the distribution image twice (maximum, then colours)
    wrote = K * T * H * W * 3 * 2
    with torch.cuda.device(pred.device):
        seq = torch.from_numpy(best.astype(np.int32)).to(pred.device)
        lut = torch.from_numpy(np.array(colormap.VIRIDIS_U8)).to(pred.device)
        f = torch.empty((K, 1, T, H, W, 3), dtype=torch.uint8, device=pred.device)
        d = torch.empty((K, 1, 1, T, H, W, 3), dtype=torch.uint8, device=pred.device)
        stream = torch.cuda.current_stream(pred.device)
        ms = []
        for i in range(warmup + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            _lib.check(pred._libh.vf_render_plans(pred._handle, seq.data_ptr(), K, lut.data_ptr(), f.data_ptr(),
                                                  d.data_ptr(), pred._stream()))
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        assert np.array_equal(f.cpu().numpy(), want['frames']) and np.array_equal(d.cpu().numpy(), want['distributions'])
    line('a', 'vf_render_plans, resident, two kernels (HIP events)', ms, calls,
         '; reads %.2f MB, writes %.2f MB' % (read / 1e6, wrote / 1e6))

    def wall(fn):
        out = []
        for i in range(warmup + calls):
            torch.cuda.synchronize(pred.device)
            t0 = time.perf_counter()
            res = fn()
            if i >= warmup:
                out.append(1e3 * (time.perf_counter() - t0))
        return out, res

    ms, res = wall(lambda: pred.render_plans(best))
    assert pred._last_M == M
    line('b', 'render_plans, resident (host clock, bytes on the host)', ms, calls, '; %.2f MB leave the device' % (wrote / 1e6))

    def rerolled():
        pred._last_M = 0            # as after a chunked or sharded scoring call: the ten are rolled again as one batch
        return pred.render_plans(best)

    ms, res2 = wall(rerolled)
    assert all(np.array_equal(res[k], want[k]) and np.array_equal(res2[k], want[k]) for k in want)
    line('b', 'render_plans, re-rolled (one 10-sequence rollout + render)', ms, calls)

    def through_call():
        out = pred(ctx, {'actions': actions})
        return colormap.render_prediction(out['predicted_frames'][best], out['predicted_pixel_distributions'][best])

    ms, res3 = wall(through_call)
    assert all(np.array_equal(res3[k], want[k]) for k in want)
    line('c', '__call__ (all %d videos to the host) + NumPy colouring of ten' % M, ms, calls,
         '; %.1f MB leave the device' % (M * T * H * W * 4 * 4 / 1e6))


class DiscardingWorker(object):
    def put(self, message):
        pass


def time_planning(calls, warmup):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    pol = {'nactions': T, 'repeat': 1, 'rejection_sampling': False}
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    pix = dict(desig_pix=[[32, 32]], goal_pix=[[16, 48]])
    worker = DiscardingWorker()
    with contextlib.redirect_stdout(io.StringIO()):
        # (verbose=True is the default, and the policy refuses an override that repeats a default)
        ctrls = {'verbose=True + discarding worker': PixelCostController(dict(ag), dict(pol), 0, 1),
                 'verbose=False': PixelCostController(dict(ag), dict(pol, verbose=False), 0, 1)}
        for c in ctrls.values():
            c.reset()
            c.act(t=0, i_tr=0, images=frames[:1], state=states[:1], verbose_worker=worker, **pix)
    ms = {name: [] for name in ctrls}
    np.random.seed(0)
    for i in range(warmup + calls):
        for name, c in ctrls.items():           # alternating: both see the same box at the same time
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                c.act(t=1, i_tr=0, images=frames, state=states, verbose_worker=worker, **pix)
            if i >= warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    for name, v in ms.items():
        line('d', 'planning call, %s' % name, v, calls)
    a, b = (np.median(v) for v in ms.values())
    print('c2 K=%d (d) the page costs %.2f ms of a planning call (%+.2f %%)' % (K, a - b, 100 * (a / b - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_plan_render.py measures on a GPU; none is visible')
    print('plan visualisation on %s, medians of %d calls after %d warm-ups; C2 = %d sequences x T%d x %dx%d, one pixel'
          % (torch.cuda.get_device_name(0), args.calls, args.warmup, M, T, H, W))
    time_render(args.calls, args.warmup)
    time_planning(args.calls, args.warmup)


if __name__ == '__main__':
    main()
