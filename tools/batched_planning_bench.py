"""What does one rollout launch for several planning problems (grouped contexts) give?  One GPU, one build, one
process, one engine per shape; the variants of a measurement are timed ALTERNATELY - ``--repeats`` (5) rounds, the order
swapped every round - and the medians over the rounds are reported with every round's figure and the spread (max - min).

1. eight problems of 25 samples (64 x 64, cdna, fp32, T13): one grouped launch against eight single-context launches of 25;
2. eleven problems of 18 samples at the towel shape (48 x 64, appearance flow, T15), the same two ways;
3. one problem of 200 rows (64 x 64, cdna, T13), grouped against broadcast: what the loss of context de-duplication costs;
4. ``vf_group_pixel_scores`` alone at those 200 rows against the reduction of the rollout's own sums (``scores_kernel`` has
   no entry of its own: ``vf_ensemble_scores`` with ONE member runs the same reads and the same reduction);
5. one ``BatchedPixelCostPlanner.act`` of eight problems (25 samples, T13, 3 iterations, Philox host sampler) against eight
   ``PixelCostController.act`` on engines of their own.

The single-context launches of 1 and 2 are timed twice: with ``vf_set_context`` of another problem's context in front of
every launch - G problems taking turns on one engine, which recomputes the context-only units every time - and with ONE
context kept (the context-only cache hits: what G engines with a context each would do, one after the other).  Times are
milliseconds between two events on the launch stream (5: wall time around the synchronised call).

    python tools/batched_planning_bench.py [--out profiles/batched_planning.txt] [--repeats 5] [--launches 10] [--quick]
"""
import argparse
import contextlib
import ctypes
import io
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def build(hp, B, T):
    from visual_foresight_amd.video_prediction.cdna_arch import CdnaWeights
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pred = HipVPredEvaluation('', dict(dict(adim=4, sdim=5, designated_pixel_count=1), run_batch_size=B,
                                       sequence_length=T + 2, **hp))
    pred.restore(CdnaWeights.random(pred.cfg, seed=3, bias_scale=0.05, ln_jitter=0.1))
    return pred


def problems(pred, G, M, T, seed=1):
    c = pred.cfg
    rs = np.random.RandomState(seed)
    contexts = []
    for _ in range(G):
        d = np.zeros((2, 1, c.height, c.width, 1), np.float32)
        d[:, :, rs.randint(0, c.height), rs.randint(0, c.width)] = 1.
        contexts.append({'context_frames': rs.randint(0, 256, (2, 1, c.height, c.width, 3)).astype(np.uint8),
                         'context_actions': rs.normal(0, 0.05, (1, c.adim)), 'context_states': rs.normal(0, 0.1, (2, c.sdim)),
                         'context_pixel_distributions': d})
    actions = rs.normal(0, 0.1, (G, M, T, c.adim)).astype(np.float32)
    goals = np.stack([rs.randint(0, c.height, (G, 1, 1)), rs.randint(0, c.width, (G, 1, 1))], axis=-1).astype(np.int32)
    return contexts, actions, goals


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(title, times, base):
    lines = [title]
    for name, ts in times.items():
        lines.append('  %-46s median %8.3f  rounds %s  spread %.3f' % (name, np.median(ts), ' '.join('%.3f' % t for t in ts), max(ts) - min(ts)))
    mb = float(np.median(times[base]))
    for name, ts in times.items():
        if name != base:
            lines.append('  %s / %s = %.3f' % (base, name, mb / float(np.median(ts))))
    return lines


def launch_shapes(name, hp, G, M, T, a):
    """Measurements 1 / 2: G problems of M rows, grouped in one launch against G single-context launches."""
    import torch
    pred = build(hp, G * M, T)
    contexts, actions, goals = problems(pred, G, M, T)
    dev = pred.device
    rows = torch.from_numpy(actions.reshape(G * M, T, -1)).to(dev)
    per = [rows[g * M:(g + 1) * M].contiguous() for g in range(G)]
    scores = torch.empty(G * M, dtype=torch.float64, device=dev)
    per_task = torch.empty((G * M, 1), dtype=torch.float64, device=dev)
    goal_dev = torch.from_numpy(goals.reshape(-1)).to(dev)

    def grouped():          # the contexts are in place: what every CEM iteration of a planning call pays
        pred._rollout_chunk(rows, goals[0], 10., scores, per_task)

    def grouped_with_cost():
        grouped()
        pred._libh.vf_group_pixel_scores(pred._handle, goal_dev.data_ptr(), ctypes.c_float(10.), None, scores.data_ptr(),
                                         per_task.data_ptr(), pred._stream())

    def grouped_with_contexts():    # ... and what its first iteration pays: the upload and expansion of the G contexts
        pred._set_contexts(contexts, M)
        grouped_with_cost()

    def singles_switching():
        for g in range(G):
            pred._ctx_key = None
            pred._set_context(contexts[g])
            pred._rollout_chunk(per[g], goals[g], 10., scores[:M], per_task[:M])

    def singles_one_context():
        for g in range(G):
            pred._rollout_chunk(per[g], goals[0], 10., scores[:M], per_task[:M])

    # grouped and broadcast mode need their own set-up: the modes are timed in blocks of a round, every block enters its mode
    def enter_grouped():
        pred._set_contexts(contexts, M)

    def enter_single():
        pred._ctx_key = None
        pred._set_context(contexts[0])

    variants = [('grouped: 1 launch of %d x %d' % (G, M), enter_grouped, grouped),
                ('grouped + vf_group_pixel_scores', enter_grouped, grouped_with_cost),
                ('grouped + vf_set_contexts + cost', enter_grouped, grouped_with_contexts),
                ('%d launches of %d, context switched' % (G, M), enter_single, singles_switching),
                ('%d launches of %d, one context (cached)' % (G, M), lambda: (enter_single(), timed(singles_one_context, 1)),
                 singles_one_context)]
    out = {v[0]: [] for v in variants}
    for r in range(a.repeats + 1):          # (round 0 warms every variant up)
        k = r % len(variants)
        for vname, enter, fn in variants[k:] + variants[:k]:
            enter()
            ms = timed(fn, a.launches)
            if r:
                out[vname].append(ms)
    assert pred.device_status() == 0
    lines = report('%s: %d problems of %d samples' % (name, G, M), out, variants[3][0])
    lines.append('  (%d x %d rows)' % (G, M))
    return lines, pred


def dedup_and_cost(a):
    """Measurements 3 / 4 at 200 rows, 64 x 64 cdna T13."""
    import torch
    B, T = (200, 13) if not a.quick else (16, 3)
    pred = build(dict(image_height=64, image_width=64) if not a.quick else dict(image_height=32, image_width=32), B, T)
    contexts, actions, goals = problems(pred, 1, B, T)
    dev = pred.device
    rows = torch.from_numpy(actions.reshape(B, T, -1)).to(dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    per_task = torch.empty((B, 1), dtype=torch.float64, device=dev)
    goal_dev = torch.from_numpy(goals.reshape(-1)).to(dev)
    members = (ctypes.c_void_p * 1)(pred._handle.value)

    def roll():
        pred._rollout_chunk(rows, goals[0], 10., scores, per_task)

    def group_cost():
        pred._libh.vf_group_pixel_scores(pred._handle, goal_dev.data_ptr(), ctypes.c_float(10.), None, scores.data_ptr(),
                                         per_task.data_ptr(), pred._stream())

    def sums_cost():
        pred._libh.vf_ensemble_scores(members, 1, ctypes.c_float(0.), ctypes.c_float(10.), None, scores.data_ptr(),
                                      per_task.data_ptr(), None, pred._stream())

    t_roll = {'grouped, 1 group of %d rows' % B: [], 'broadcast, %d rows (context cached)' % B: []}
    t_cost = {'vf_group_pixel_scores, %d rows' % B: [], 'reduction of the rollout\'s sums (1-member vf_ensemble_scores)': []}
    names_r, names_c = list(t_roll), list(t_cost)
    for r in range(a.repeats + 1):
        for mode in ((0, 1) if r % 2 == 0 else (1, 0)):
            if mode == 0:
                pred._set_contexts(contexts, B)
            else:
                pred._ctx_key = None
                pred._set_context(contexts[0])
            timed(roll, 2)
            ms = timed(roll, a.launches)
            if r:
                t_roll[names_r[mode]].append(ms)
            if mode == 0:       # the last rollout is a grouped one: both reductions read it
                for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                    fn = group_cost if which == 0 else sums_cost
                    timed(fn, 2)
                    ms = timed(fn, 10 * a.launches)
                    if r:
                        t_cost[names_c[which]].append(ms)
    assert pred.device_status() == 0
    c = pred.cfg
    mb = B * T * c.height * c.width * 4 / 1e6
    lines = report('3. one problem of %d rows, %d x %d cdna T%d: grouped against broadcast' % (B, c.height, c.width, T), t_roll, names_r[1])
    lines += ['']
    lines += report('4. the grouped cost alone at those %d rows (one pass over %.1f MB of distributions)' % (B, mb), t_cost, names_c[1])
    med = float(np.median(t_cost[names_c[0]]))
    lines.append('  -> %.0f GB/s over the resident distributions' % (mb / med))
    return lines


def planner_call(a):
    """Measurement 5: one BatchedPixelCostPlanner.act of G problems against G PixelCostController.act."""
    import torch
    from visual_foresight_amd.policy.cem_controllers import BatchedPixelCostPlanner, PixelCostController
    from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import PhiloxGaussianCEMSampler
    G, M, T, H, W = (8, 25, 13, 64, 64) if not a.quick else (3, 12, 3, 32, 32)
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}

    def pol(seed):
        return dict(verbose=False, sampler=PhiloxGaussianCEMSampler, device_cem=False, nactions=T, repeat=1, num_samples=M,
                    sampler_seed=seed, minimum_selection=5)

    def request(g, t):
        rs = np.random.RandomState(300 + g)
        images = rs.randint(0, 256, (3, 1, H, W, 3)).astype(np.uint8)
        states = rs.normal(0, 0.1, (3, 5))
        pix = rs.randint(0, min(H, W), (2, 1, 2))
        return dict(t=t, i_tr=0, desig_pix=pix[0], goal_pix=pix[1], images=images[:t + 1], state=states[:t + 1])

    with contextlib.redirect_stdout(io.StringIO()):
        planner = BatchedPixelCostPlanner(ag, [pol(20 + g) for g in range(G)], 0, 1, G)
        singles = [PixelCostController(ag, pol(20 + g), 0, 1) for g in range(G)]
        t_b, t_s = [], []
        for r in range(a.repeats + 1):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                if which == 0:      # (step 0 lies below start_planning: it logs the action the context of step 1 holds)
                    planner.reset()
                    planner.act([request(g, 0) for g in range(G)])
                else:
                    for g, c in enumerate(singles):
                        c.reset()
                        c.act(**request(g, 0))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == 0:
                    planner.act([request(g, 1) for g in range(G)])
                else:
                    for g, c in enumerate(singles):
                        c.act(**request(g, 1))
                torch.cuda.synchronize()
                if r:
                    (t_b if which == 0 else t_s).append(1e3 * (time.perf_counter() - t0))
    assert planner.predictor.device_status() == 0
    times = {'BatchedPixelCostPlanner.act, %d problems' % G: t_b, '%d PixelCostController.act' % G: t_s}
    return report('5. one planning call (3 CEM iterations, %d samples, T%d, %d x %d, Philox host sampler): wall ms' % (M, T, H, W),
                  times, '%d PixelCostController.act' % G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'batched_planning.txt'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='small shapes: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    lines = ['several planning problems in one rollout launch: grouped contexts (tools/batched_planning_bench.py)',
             'device: %s; %d rounds of %d calls per variant, alternating, after a warm-up round; ms per call'
             % (torch.cuda.get_device_name(0), a.repeats, a.launches), '']
    warm = build(dict(image_height=32, image_width=32), 1, 3)     # (the first engine of a process pays for loading the code object)
    if a.quick:
        shapes = [('1. quick 32 x 32 cdna T3', dict(image_height=32, image_width=32), 3, 4, 3),
                  ('2. quick 48 x 64 flow T3', dict(image_height=48, image_width=64, transformation='flow'), 2, 3, 3)]
    else:
        shapes = [('1. 64 x 64 cdna fp32 T13', dict(image_height=64, image_width=64), 8, 25, 13),
                  ('2. towel 48 x 64 flow T15', dict(image_height=48, image_width=64, transformation='flow'), 11, 18, 15)]
    for name, hp, G, M, T in shapes:
        part, pred = launch_shapes(name, hp, G, M, T, a)
        lines += part + ['']
        print('\n'.join(part), flush=True)
        del pred
    for part in (dedup_and_cost(a), planner_call(a)):
        lines += part + ['']
        print('\n'.join(part), flush=True)
    del warm
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
