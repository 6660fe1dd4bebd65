#!/usr/bin/env python
"""Time the STP predictor against the cdna and the appearance-flow predictor on the GPU (``--out profiles/stp.txt`` appends
the report to that file, behind the parity figures it holds) - or, with ``--helper-distance``, measure on the CPU how far
the float32 helper oracle of the STP tests lies from its own float64 mode (section 1 of that file).

At the C2 shape (200 sequences x T13 x 64 x 64, one designated pixel, seeded random weights) it reports

  (a) one rollout + cost reduction (``score``) of a ``transformation='stp'``, a ``'cdna'`` and a ``'flow'`` engine of the same
      commit, in the same process, alternating call by call and rotating the order: host clock around a call that ends in
      a device synchronise, median / min / max over ``--calls`` calls after ``--warmup`` warm-ups (the context is cached
      after the first call, as in the CEM iterations of a planning call);
  (b) per phase type of the persistent schedule (``vf_set_phase_stats``): items, and the wall-clock ticks its items spent
      running, summed over the launch - the fused top (transposed conv + compositing) of the three engines side by side,
      the FC and the finish items of the cdna and the stp engine;
  (c) the work the stp compositing adds and drops, counted from the shapes.

    python tools/stp_bench.py [--calls 15] [--warmup 3] [--out profiles/stp.txt]
    python tools/stp_bench.py --helper-distance [--out profiles/stp.txt]        (CPU only)
"""
import argparse
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

H = W = 64
T, M, ND = 13, 200, 1
PHASE_NAMES = {0: 'conv-LSTM', 1: 'conv+relu', 2: 'conv raw', 3: 'convT+relu', 4: 'convT raw', 5: 'FC (K splits)', 6: 'state FC',
               7: 'kernel finish', 8: 'compositing', 9: 'fused top', 10: 'enc2+enc3', 13: 'recurrent partial',
               17: 'stp finish'}


def make(transformation):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=ND, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, transformation=transformation)
    pred = HipVPredEvaluation('', hp)
    pred.restore()
    return pred


def phase_stats(pred):
    """{phase type: [phases, items, wait ticks, run ticks]} of the last persistent rollout."""
    n_max = 4096
    types, items = (ctypes.c_int32 * n_max)(), (ctypes.c_int32 * n_max)()
    wr = (ctypes.c_uint64 * (2 * n_max))()
    n = pred._libh.vf_debug_phase_stats(pred._handle, n_max, types, items, wr)
    assert n > 0, 'no phase statistics'
    out = {}
    for i in range(n):
        row = out.setdefault(types[i], [0, 0, 0, 0])
        row[0] += 1; row[1] += items[i]; row[2] += wr[2 * i]; row[3] += wr[2 * i + 1]
    return out


def helper_distance(say):
    """The float32 helper against its float64 mode at the inputs of tests/test_gpu_stp.py's two parity tests (CPU)."""
    import torch
    from oracle import pixel_cost
    from tests import test_gpu_stp as t
    from tests.helpers.oracle_stp import OracleStp
    worst = {}
    for head_out in (True, False):
        say('   %s' % ('head taken out (stp_fc/w = stp/w = 0, nine fixed transforms):' if head_out
                       else 'every tensor random, stp/w scaled by %.2f:' % t.STP_W_SCALE))
        say('   shape (H x W, nd, context frames)   frames     distrib/planemax   states     scores rel   max |theta - identity|')
        for (Hh, Ww, nc, Tt, Mm, nd) in t.PARITY_CASES:
            weights, ctx, actions, goal = t.parity_inputs(Hh, Ww, Tt, Mm, nd, nc, head_out)
            out, dev = [], 0.0
            for dtype in (torch.float32, torch.float64):
                ora = OracleStp(weights, dtype)
                f, d, s = ora.rollout(ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'],
                                      ctx['context_states'], actions)
                dev = float((ora.last_theta - torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)).abs().max())
                out.append((f, d, s, pixel_cost.eval_pixel_cost(d, goal, 10.)[0]))
            (f0, d0, s0, c0), (f1, d1, s1, c1) = out
            e = dict(frames=np.abs(f0 - f1).max(), distrib=(np.abs(d0 - d1) / d1.max(axis=(3, 4), keepdims=True)).max(),
                     states=np.abs(s0 - s1).max(), scores=np.abs(c0 / c1 - 1).max())
            say('   %dx%d  nd %d  nc %d  (T %d, M %d)       %.2e   %.2e           %.2e   %.2e     %.3f'
                % (Hh, Ww, nd, nc, Tt, Mm, e['frames'], e['distrib'], e['states'], e['scores'], dev))
            if not head_out:
                for k, v in e.items():
                    worst[k] = max(worst.get(k, 0.0), float(v))
    say('   largest over the ten full-parity cases: ' + ', '.join('%s %.2e' % (k, worst[k]) for k in ('frames', 'distrib', 'states', 'scores')))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default='')
    ap.add_argument('--helper-distance', action='store_true')
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, 'a') as f:
                f.write('\n'.join(lines) + '\n')

    if args.helper_distance:
        helper_distance(say)
        return flush()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    rs = np.random.RandomState(0)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': None}
    from oracle import pixel_cost
    ctx['context_pixel_distributions'] = pixel_cost.one_hot_distrib([[[32, 32]]], 2, 1, H, W, ND)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = np.array([[[16, 48]]])
    ORDER = ('stp', 'cdna', 'flow')
    preds = {name: make(name) for name in ORDER}
    times = {name: [] for name in preds}
    first = {}
    for i in range(args.warmup + args.calls):
        for name in ORDER[i % 3:] + ORDER[:i % 3]:          # alternate, and rotate the order
            pred = preds[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s, _ = pred.score(ctx, {'actions': actions}, goal)      # ends in a device-to-host copy of the scores
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                times[name].append(dt)
            if name not in first:
                first[name] = s
            assert np.array_equal(first[name], s), 'repeated rollouts must reproduce their scores'
    say('stp vs cdna vs appearance flow, %d sequences x T%d x %dx%d, nd %d, one rollout + cost reduction (score), host clock'
        % (M, T, H, W, ND))
    say('around a synchronised call, %d calls after %d warm-ups, the three engines alternating in one process:'
        % (args.calls, args.warmup))
    med = {}
    for name in ('cdna', 'flow', 'stp'):
        ms = np.asarray(times[name])
        med[name] = float(np.median(ms))
        say('  (a) %-4s  median %.3f ms  (min %.3f, max %.3f)  %.0f sample-steps/s' %
            (name, med[name], ms.min(), ms.max(), M * T / med[name] * 1e3))
        assert preds[name].device_status() == 0
    say('      stp / cdna = %.4f, stp / flow = %.4f, flow / cdna = %.4f'
        % (med['stp'] / med['cdna'], med['stp'] / med['flow'], med['flow'] / med['cdna']))
    say('  (b) phases of one persistent launch (cached context), wall-clock ticks summed over the items of a type:')
    stats = {}
    for name, pred in preds.items():
        from visual_foresight_amd import _lib
        _lib.check(pred._libh.vf_set_phase_stats(pred._handle, 1))
        pred.score(ctx, {'actions': actions}, goal)
        stats[name] = phase_stats(pred)
        _lib.check(pred._libh.vf_set_phase_stats(pred._handle, 0))
    say('      %-18s %28s   %28s   %28s' % ('', 'cdna: items, run ticks, /item', 'flow: items, run ticks, /item',
                                             'stp: items, run ticks, /item'))
    for t in sorted(set(stats['cdna']) | set(stats['flow']) | set(stats['stp'])):
        cells = []
        for name in ('cdna', 'flow', 'stp'):
            r = stats[name].get(t)
            cells.append('%8d %12d %7.0f' % (r[1], r[3], r[3] / max(r[1], 1)) if r else '%28s' % '-')
        say('      %-18s %s   %s   %s' % (PHASE_NAMES.get(t, 'type %d' % t), cells[0], cells[1], cells[2]))
    tot = {name: sum(r[3] for r in stats[name].values()) for name in stats}
    say('      all phases: run ticks cdna %d, flow %d, stp %d (stp / cdna = %.4f, stp / flow = %.4f)'
        % (tot['cdna'], tot['flow'], tot['stp'], tot['stp'] / tot['cdna'], tot['stp'] / tot['flow']))
    say('  (c) counted from the shapes: per pixel the stp compositing gathers %d taps (nine warps x four taps x (3 + nd) channels)'
        % (9 * 4 * (3 + ND)))
    say('      where cdna runs %d tap MACs over its LDS halo and flow adds a %d-MAC head in front of the same gathers; per'
        % (25 * 9 + 25 * (3 + ND), 32 * 18))
    say('      sample-step the first FC is %.2f MMAC (cdna FC %.2f) and the finish item adds %d MACs.'
        % ((H // 8) * (W // 8) * 128 * 100 / 1e6, (H // 8) * (W // 8) * 128 * 250 / 1e6, 100 * 54))
    flush()


if __name__ == '__main__':
    main()
