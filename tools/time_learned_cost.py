#!/usr/bin/env python
"""Time the learned cost on the GPU (profiles/learned_cost.txt is this tool's output).

At C2 (200 sequences x T13 x 64x64), at the C4 share (125 x T15 x 64x64) and at 128x128 (125 x T15), for both heads, it
reports as medians of 20 calls after 5 warm-ups:

  (a) one scoring pass - ``vf_scorer_scores`` on the frames of the last rollout, HIP events around the call on the
      rollout's stream, a rollout in front of every timed call as a planning call has - with the FLOPs executed on the
      matrix pipe and the vector ALU (padding taps and idle MFMA rows included), their fraction of the 157.3 TFLOP/s fp32
      peak, and the frame bytes read;
  (b) at C2, what the same frames cost on the only other route to a learned cost: ``vf_export`` + the device-to-host copy
      (host clock around work that ends in a synchronise), and the CPU oracle scorer on the exported frames beside it;
  (c) at C2, one planning call (3 CEM iterations) of ``ClassifierController`` and of ``PixelCostController``, alternating
      in the same process, host clock around ``act``.

It also prints the head-output errors of the device, of the float32 oracle and of the float32 chain in the device's K
order against the float64 oracle on rolled frames (the figures behind tests/test_gpu_learned_cost.py's bound).

    python tools/time_learned_cost.py [--calls 20] [--warmup 5]
"""
import argparse
import contextlib
import ctypes
import io
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = {'c2': dict(H=64, W=64, T=13, actions=200), 'c4share': dict(H=64, W=64, T=15, actions=125),
          '128x128': dict(H=128, W=128, T=15, actions=125)}


def make(shape, head):
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    s = SHAPES[shape]
    hp = dict(designated_pixel_count=1, run_batch_size=s['actions'], adim=4, sdim=5, image_height=s['H'],
              image_width=s['W'], sequence_length=s['T'] + 2)
    pred = HipVPredEvaluation('', hp).restore()
    scorer = HipFrameScorer('', dict(image_height=s['H'], image_width=s['W'], head=head, max_frames=s['actions'] * s['T'],
                                     bias_scale=0.2), pred.device).restore()
    rs = np.random.RandomState(0)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, s['H'], s['W'], 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5))}
    actions = rs.normal(0, 0.1, (s['actions'], s['T'], 4))
    goal_enc = None
    if head == 'embedding':
        goal_enc = scorer.goal_enc(rs.uniform(0, 1, (1, s['H'], s['W'], 3)), ctx['context_frames'][-1] / 255.)
    return pred, scorer, ctx, actions, goal_enc


def executed_flops(H, W, D):
    """FLOPs the kernels execute per frame: c1 on the vector ALU, c2 - c4 as whole 32-row MFMA tiles, the head."""
    valu = 2 * (H // 2) * (W // 2) * 27 * 32 + 2 * 128 * D + (H // 16) * (W // 16) * 128
    mfma, cin = 0, 32
    for l, cout in ((2, 64), (3, 128), (4, 128)):
        P = (H >> l) * (W >> l)
        mfma += 2 * ((P + 31) // 32) * 32 * 9 * cin * cout
        cin = cout
    return valu, mfma


def med_spread(ms):
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def time_pass(shape, head, calls, warmup):
    import torch
    from visual_foresight_amd import _lib
    s = SHAPES[shape]
    pred, scorer, ctx, actions, goal_enc = make(shape, head)
    want = pred.score_frames(ctx, {'actions': actions}, scorer, goal_enc=goal_enc)
    n = s['actions']
    with torch.cuda.device(pred.device):
        g = None if goal_enc is None else torch.from_numpy(goal_enc).to(pred.device)
        out = torch.empty(n, dtype=torch.float64, device=pred.device)
        stream = torch.cuda.current_stream(pred.device)
        seqs = torch.from_numpy(np.ascontiguousarray(pred._last_prepared[1], dtype=np.float32)).to(pred.device)
        r_s = torch.empty(n, dtype=torch.float64, device=pred.device)
        r_pt = torch.empty((n, 1), dtype=torch.float64, device=pred.device)
        ms = []
        for i in range(warmup + calls):
            pred._rollout_chunk(seqs, [[[s['H'] // 2, s['W'] // 2]]], 1.0, r_s, r_pt)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            _lib.check(pred._libh.vf_scorer_scores(scorer._handle, pred._handle, None if g is None else g.data_ptr(),
                                                   ctypes.c_float(100.), out.data_ptr(), None, None, pred._stream()))
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        assert np.array_equal(out.cpu().numpy(), want), 'the timed calls must reproduce the scores'
    med, lo, hi = med_spread(ms)
    frames = n * s['T']
    valu, mfma = executed_flops(s['H'], s['W'], scorer.cfg.out_dim)
    tf = frames * (valu + mfma) / med / 1e9
    print('%-8s (a) %-10s one scoring pass right after a rollout, %d frames: median %.3f ms (min %.3f, max %.3f) over %d '
          'calls; executed %.1f GFLOP (%.1f MFMA + %.1f VALU) -> %.1f TFLOP/s = %.1f %% of %.1f; reads %.1f MB of frames'
          % (shape, head, frames, med, lo, hi, calls, frames * (valu + mfma) / 1e9, frames * mfma / 1e9, frames * valu / 1e9,
             tf, 100 * tf / PEAK_TFLOPS, PEAK_TFLOPS, frames * s['H'] * s['W'] * 12 / 1e6))
    return pred, scorer, med


def time_export_route(pred, scorer, calls, warmup, pass_ms):
    """(b): export + device-to-host copy of the frames of the last rollout, and the CPU oracle scorer on them."""
    import torch
    from tests.helpers import oracle_frame_scorer as ora
    from visual_foresight_amd import _lib
    s = SHAPES['c2']
    B = s['actions']
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
            if i >= warmup:
                parts.append((t1 - t0, t2 - t1, t2 - t0))
    med = np.median(np.array(parts), axis=0) * 1e3
    t0 = time.perf_counter()
    enc = ora.forward_views(scorer.weights['frames'], host.reshape((-1,) + host.shape[2:]), scorer.cfg.input_scale,
                            torch.float32)
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    print('c2       (b) the route without the scorer: vf_export %.2f ms + device-to-host copy of %.1f MB %.2f ms = median '
          '%.1f ms over %d calls, before a frame is scored; the CPU oracle scorer (float32, %d threads) on those frames: '
          '%.0f ms' % (med[0], f.numel() * 4 / 1e6, med[1], med[2], calls, torch.get_num_threads(), cpu_ms))
    print('c2       requirement: scoring pass %.3f ms < export + copy %.1f ms: %s (%.0f x)'
          % (pass_ms, med[2], 'MET' if pass_ms < med[2] else 'NOT MET', med[2] / pass_ms))
    return host, enc


def head_errors(pred, scorer, host):
    import torch
    from tests.helpers import oracle_frame_scorer as ora
    _, _, head_out = pred.score_resident_frames(scorer, None, 100.)
    flat = host.reshape((-1,) + host.shape[2:])[:64]
    dev = head_out.reshape(-1, 1, head_out.shape[-1])[:64]
    f64 = ora.forward_views(scorer.weights['frames'], flat, scorer.cfg.input_scale, torch.float64)
    f32 = ora.forward_views(scorer.weights['frames'], flat, scorer.cfg.input_scale, torch.float32)
    chain = ora.forward_device_order(scorer.weights['frames'][0], flat[:, 0], scorer.cfg.input_scale)[:, None]
    top = np.abs(f64).max()
    e = [np.abs(x.astype(np.float64) - f64).max() / top for x in (dev, f32, chain)]
    print('c2       head outputs of 64 rolled frames against the float64 oracle (max abs error / largest |output|): device '
          '%.3g, float32 oracle %.3g, float32 chain in the device\'s K order %.3g; bound of the test: 8 x the float32 '
          'oracle\'s figure = %.3g' % (e[0], e[1], e[2], 8 * e[1]))


def time_planning(calls, warmup):
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController
    s = SHAPES['c2']
    ag = {'adim': 4, 'sdim': 5, 'image_height': s['H'], 'image_width': s['W']}
    pol = {'nactions': s['T'], 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, s['H'], s['W'], 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    with contextlib.redirect_stdout(io.StringIO()):
        ctrls = {'ClassifierController': ClassifierController(dict(ag), dict(pol), 0, 1),
                 'PixelCostController': PixelCostController(dict(ag), dict(pol), 0, 1)}
        kwargs = {'ClassifierController': {}, 'PixelCostController': dict(desig_pix=[[32, 32]], goal_pix=[[16, 48]])}
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
        print('c2       (c) %-20s planning call (200 x T13 x 64x64, 3 iterations): median %.2f ms (min %.2f, max %.2f) '
              'over %d calls' % (name, med, lo, hi, calls))
    c, p = stats['ClassifierController'][0], stats['PixelCostController'][0]
    print('c2       (c) ClassifierController - PixelCostController = %.2f ms per call, %.2f ms per iteration' % (c - p, (c - p) / 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_learned_cost.py measures on a GPU; none is visible')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    print('learned cost on %s, medians of %d calls after %d warm-ups' % (torch.cuda.get_device_name(0), args.calls, args.warmup))
    for shape in SHAPES:
        for head in ('classifier', 'embedding'):
            pred, scorer, med = time_pass(shape, head, args.calls, args.warmup)
            if shape == 'c2' and head == 'classifier':
                host, _ = time_export_route(pred, scorer, args.calls, args.warmup, med)
                head_errors(pred, scorer, host)
            del pred, scorer
            sys.stdout.flush()
    time_planning(args.calls, args.warmup)


if __name__ == '__main__':
    main()
