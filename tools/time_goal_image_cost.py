#!/usr/bin/env python
"""Time the goal-image cost on the GPU (profiles/goal_image_cost.txt is this tool's output).

At C2 (200 sequences x T13 x 64x64, cdna) and at the 125-sequence 128x128 share (25 actions x 5 latent draws, T15, savp)
it reports, as medians of 20 calls after 5 warm-ups:

  (a) ``vf_goal_image_scores`` alone in both modes, HIP events around the call on the rollout's stream, with the bytes the
      reduction reads (frames + goal) and the resulting GB/s and fraction of the 6.3 TB/s streaming rate - first back
      to back (every call re-reads the frames the previous one read: up to 256 MB of them are served by the last-level
      cache, so that rate is not an HBM rate), then with a rollout in front of every timed call, as a planning call has;
  (b) what the same cost takes without that entry point: ``vf_export`` of the frames + device-to-host copy + the NumPy
      reduction, host clock around work that ends in a synchronise.  ``--baseline-library PATH`` runs (b) in a child
      process on another build of the library (the parent commit's, which lacks the new export; (b) never calls it);
  (c) at C2, one planning call (3 CEM iterations) of ``GoalImController`` and of ``PixelCostController``, alternating in
      the same process, host clock around ``act``, with the spread of each.

    python tools/time_goal_image_cost.py [--baseline-library PATH] [--calls 20] [--warmup 5]
"""
import argparse
import contextlib
import ctypes
import io
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

PEAK_GBS = 6300.0
SHAPES = {'c2': dict(arch='cdna', H=64, W=64, T=13, actions=200, n_latent=0),
          'c5share': dict(arch='savp', H=128, W=128, T=15, actions=25, n_latent=5)}


def make_predictor(shape):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor
    s = SHAPES[shape]
    hp = dict(designated_pixel_count=1, run_batch_size=s['actions'], adim=4, sdim=5, image_height=s['H'],
              image_width=s['W'], sequence_length=s['T'] + 2)
    if s['n_latent']:
        hp.update(arch=s['arch'], n_latent=s['n_latent'], zdim=8)
        pred = StochasticHipPredictor('', hp)
    else:
        pred = HipVPredEvaluation('', hp)
    pred.restore()
    rs = np.random.RandomState(0)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, s['H'], s['W'], 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5))}
    actions = rs.normal(0, 0.1, (s['actions'], s['T'], 4))
    goal = rs.randint(0, 256, (1, s['H'], s['W'], 3)).astype(np.uint8)
    return pred, ctx, actions, goal


def med_spread(ms):
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def time_entry(shape, calls, warmup):
    import torch
    from visual_foresight_amd import _lib
    s = SHAPES[shape]
    pred, ctx, actions, goal = make_predictor(shape)
    B = s['actions'] * max(s['n_latent'], 1)
    img = s['H'] * s['W'] * 3 * 4
    want, _ = pred.score_goal_image(ctx, {'actions': actions}, goal, steps='weighted')       # rolls; frames stay resident
    with torch.cuda.device(pred.device):
        g = torch.from_numpy(goal.astype(np.float32) / np.float32(255.)).to(pred.device)
        out = torch.empty(s['actions'], dtype=torch.float64, device=pred.device)
        stream = torch.cuda.current_stream(pred.device)
        for mode, name, steps in ((0, 'last step', 1), (1, 'weighted', s['T'])):
            ms = []
            for i in range(warmup + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                _lib.check(pred._libh.vf_goal_image_scores(pred._handle, g.data_ptr(), mode, ctypes.c_float(10.), 0,
                                                           out.data_ptr(), None, None, pred._stream()))
                b.record(stream)
                b.synchronize()
                if i >= warmup:
                    ms.append(a.elapsed_time(b))
            med, lo, hi = med_spread(ms)
            nbytes = B * steps * img + img
            print('%-8s (a) vf_goal_image_scores %-9s back to back: median %.4f ms (min %.4f, max %.4f) over %d calls; '
                  'reads %.2f MB -> %.0f GB/s = %.1f %% of %.1f TB/s'
                  % (shape, name, med, lo, hi, calls, nbytes / 1e6, nbytes / 1e6 / med,
                     100 * nbytes / 1e6 / med / PEAK_GBS, PEAK_GBS / 1e3))
        assert np.array_equal(out.cpu().numpy(), want), 'the timed calls must reproduce the scores'
        # in place: each timed call follows a rollout on the same stream, as in a planning call - the frames are
        # where the persistent launch left them, not in a cache warmed by the previous timed call
        seqs = torch.from_numpy(np.ascontiguousarray(pred._last_prepared[1], dtype=np.float32)).to(pred.device)
        r_s = torch.empty(s['actions'], dtype=torch.float64, device=pred.device)
        r_pt = torch.empty((s['actions'], 1), dtype=torch.float64, device=pred.device)
        for mode, name in ((0, 'last step'), (1, 'weighted')):
            ms = []
            for i in range(warmup + calls):
                pred._rollout_chunk(seqs, [[[s['H'] // 2, s['W'] // 2]]], 1.0, r_s, r_pt)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                _lib.check(pred._libh.vf_goal_image_scores(pred._handle, g.data_ptr(), mode, ctypes.c_float(10.), 0,
                                                           out.data_ptr(), None, None, pred._stream()))
                b.record(stream)
                b.synchronize()
                if i >= warmup:
                    ms.append(a.elapsed_time(b))
            med, lo, hi = med_spread(ms)
            print('%-8s (a) ... %-9s right after a rollout: median %.4f ms (min %.4f, max %.4f) over %d calls'
                  % (shape, name, med, lo, hi, calls))
        assert np.array_equal(out.cpu().numpy(), want), 'the timed calls must reproduce the scores'


def time_baseline(shape, calls, warmup, tag):
    """(b): export + device-to-host copy + NumPy, on whatever library this process loaded."""
    import torch
    from visual_foresight_amd import _lib
    s = SHAPES[shape]
    pred, ctx, actions, goal = make_predictor(shape)
    nl = max(s['n_latent'], 1)
    B = s['actions'] * nl
    goal_f = (goal.astype(np.float32) / np.float32(255.)).astype(np.float64)
    pred.score(dict(ctx, context_pixel_distributions=_centre(s, pred)), {'actions': actions},
               [[[s['H'] // 2, s['W'] // 2]]])                                              # rolls; frames stay resident
    w = np.ones(s['T'])
    w[-1] = 10.
    parts = []
    with torch.cuda.device(pred.device):
        f = torch.empty((B, s['T'], 1, s['H'], s['W'], 3), dtype=torch.float32, device=pred.device)
        for i in range(warmup + calls):
            torch.cuda.synchronize(pred.device)
            t0 = time.perf_counter()
            _lib.check(pred._libh.vf_export(pred._handle, 0, B, f.data_ptr(), None, None, pred._stream()))
            torch.cuda.synchronize(pred.device)
            t1 = time.perf_counter()
            host = f.cpu().numpy()
            t2 = time.perf_counter()
            mse = ((host.astype(np.float64) - goal_f[None, None]) ** 2).mean(axis=(3, 4, 5))[:, :, 0]        # [B, T]
            scores = ((mse * w).sum(axis=1) / w.sum()).reshape(s['actions'], nl).mean(axis=1)
            t3 = time.perf_counter()
            if i >= warmup:
                parts.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
    med = np.median(np.array(parts), axis=0) * 1e3
    print('%-8s (b) without the entry point (%s): vf_export %.2f ms + device-to-host copy of %.1f MB %.2f ms + NumPy '
          'reduction %.1f ms = median %.1f ms over %d calls (weighted mode; score[0] = %.17g)'
          % (shape, tag, med[0], f.numel() * 4 / 1e6, med[1], med[2], med[3], calls, scores[0]))


def _centre(s, pred):
    d = np.zeros((2, 1, s['H'], s['W'], 1), np.float32)
    d[:, :, s['H'] // 2, s['W'] // 2] = 1.0
    return d


def time_planning(calls, warmup):
    from visual_foresight_amd.policy.cem_controllers import GoalImController, PixelCostController
    s = SHAPES['c2']
    ag = {'adim': 4, 'sdim': 5, 'image_height': s['H'], 'image_width': s['W']}
    pol = {'nactions': s['T'], 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, s['H'], s['W'], 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal = rs.randint(0, 256, (s['H'], s['W'], 3)).astype(np.uint8)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrls = {'GoalImController': GoalImController(dict(ag), dict(pol), 0, 1),
                 'PixelCostController': PixelCostController(dict(ag), dict(pol), 0, 1)}
        kwargs = {'GoalImController': dict(goal_image=goal),
                  'PixelCostController': dict(desig_pix=[[32, 32]], goal_pix=[[16, 48]])}
        for name, c in ctrls.items():
            c.reset()
            c.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kwargs[name])
    ms = {name: [] for name in ctrls}
    np.random.seed(0)
    for i in range(warmup + calls):
        for name, c in ctrls.items():           # alternating: both see the same box at the same time
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                c.act(t=1, i_tr=0, images=frames, state=states, **kwargs[name])
            if i >= warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    stats = {name: med_spread(v) for name, v in ms.items()}
    for name, (med, lo, hi) in stats.items():
        print('c2       (c) %-19s planning call (200 x T13 x 64x64, 3 iterations): median %.2f ms (min %.2f, max %.2f, '
              'spread %.2f %%) over %d calls' % (name, med, lo, hi, 100 * (hi - lo) / med, calls))
    g, p = stats['GoalImController'][0], stats['PixelCostController'][0]
    print('c2       (c) GoalImController / PixelCostController = %.4f (%+.2f %%)' % (g / p, 100 * (g / p - 1)))


class _WithoutNewExport(ctypes.CDLL):
    """The parent commit's library has no vf_goal_image_scores; the baseline path never calls it."""
    def __getattr__(self, name):
        try:
            return super(_WithoutNewExport, self).__getattr__(name)
        except AttributeError:
            if name != 'vf_goal_image_scores':
                raise
            return type('missing', (), {})()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline-library', default=None)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--baseline-child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_goal_image_cost.py measures on a GPU; none is visible')
    if args.baseline_child:
        ctypes.CDLL = _WithoutNewExport
        for shape in SHAPES:
            time_baseline(shape, args.calls, args.warmup, args.baseline_child)
        return
    print('goal-image cost on %s, medians of %d calls after %d warm-ups' % (torch.cuda.get_device_name(0), args.calls,
                                                                           args.warmup))
    for shape in SHAPES:
        time_entry(shape, args.calls, args.warmup)
    if args.baseline_library:
        env = dict(os.environ, VF_LIBRARY=os.path.abspath(args.baseline_library))
        sys.stdout.flush()
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--calls', str(args.calls), '--warmup',
                               str(args.warmup), '--baseline-child', 'the library given as --baseline-library'], env=env)
    else:
        for shape in SHAPES:
            time_baseline(shape, args.calls, args.warmup, 'this build')
    time_planning(args.calls, args.warmup)


if __name__ == '__main__':
    main()
