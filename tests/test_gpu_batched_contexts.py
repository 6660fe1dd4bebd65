"""Grouped contexts on the GPU (``vf_set_contexts`` / ``vf_group_pixel_scores`` / ``score_batch`` / ``BatchedPixelCostPlanner``):
G planning problems with their own contexts and goals in ONE rollout launch.

1. the rollout of G contexts x m rows is, bit for bit, G single-context rollouts of m rows - for every compositing table,
   precision and launch route;
2. the grouped cost against the reference-pinned cost applied to the engine's own exported distributions (rtol 2e-6: both
   divide by the same S0 and every term is non-negative, so the float32 rounding of the exported values bounds the
   difference - the bound ``test_gpu_parity.py::test_rollout_matches_oracle`` holds ``vf_rollout``'s scores to);
3. one case against ``OracleCdna``, at that test's tolerances;
4. the planner against its controllers planning alone on the same engine;
5. the refusals.
"""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                           # noqa: E402
from oracle.cdna_predictor import OracleCdna                            # noqa: E402
from visual_foresight_amd import _lib                                   # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaWeights    # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation     # noqa: E402


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def parity_weights(cfg, seed):
    """Random weights as ``tests/test_gpu_parity.py::_predictor`` draws them (an STP head's second FC scaled as
    ``tests/test_gpu_stp.py`` scales it, so that its warps stay near the identity)."""
    w = CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)
    if 'stp/w' in w.tensors:
        w.tensors['stp/w'] *= np.float32(0.1)
    return w


def _predictor(H, W, T, nd, bs, n_context=2, seed=3, **extra):
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + n_context, n_context=n_context, **extra)
    pred = HipVPredEvaluation('', hp)
    ws = [parity_weights(pred.cfg, seed + v) for v in range(pred.n_cam)]
    pred.restore(ws if pred.n_cam > 1 else ws[0])
    return pred, ws


def _context(H, W, nd, ncam, nc, rs):
    hist = nc + 1
    desig = np.stack([rs.randint(0, H, (ncam, nd)), rs.randint(0, W, (ncam, nd))], axis=-1)
    ctx = {'context_frames': rs.randint(0, 256, (hist, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (hist - 1, 4)),
           'context_states': rs.normal(0, 0.1, (hist, 5))}
    if nd > 0:
        ctx['context_pixel_distributions'] = pixel_cost.one_hot_distrib(desig, nc, ncam, H, W, nd)
    return ctx


def _export(pred, n):
    c, T = pred.cfg, pred.sequence_length - pred.n_context
    f = torch.empty((n, T, pred.n_cam, c.height, c.width, 3), dtype=torch.float32, device=pred.device)
    d = None if pred.frames_only else torch.empty((n, T, pred.n_cam, c.height, c.width, c.ndesig), dtype=torch.float32,
                                                  device=pred.device)
    s = torch.empty((n, T, c.sdim), dtype=torch.float32, device=pred.device)
    _lib.check(pred._libh.vf_export(pred._handle, 0, n, f.data_ptr(), None if d is None else d.data_ptr(), s.data_ptr(),
                                    pred._stream()))
    return f.cpu().numpy(), None if d is None else d.cpu().numpy(), s.cpu().numpy()


def _roll(pred, actions, goal, finalweight=10.):
    """One ``vf_rollout`` of ``actions [n, T, adim]`` in whatever mode the handle is -> (frames, distrib, states, scores,
    per_task) on the host."""
    n = actions.shape[0]
    ntask = pred.n_cam * pred.cfg.ndesig
    with torch.cuda.device(pred.device):
        seqs = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)).to(pred.device)
        scores = torch.zeros(n, dtype=torch.float64, device=pred.device)
        per_task = torch.zeros((n, ntask), dtype=torch.float64, device=pred.device)
        pred._rollout_chunk(seqs, goal, finalweight, scores, per_task)
        out = _export(pred, n) + (scores.cpu().numpy(), per_task.cpu().numpy())
    assert pred.device_status() == 0
    return out


def roll_grouped(pred, contexts, actions, goal):
    """G contexts x m rows, ``actions [G, m, T, adim]``, in grouped mode."""
    G, m = actions.shape[:2]
    pred._set_contexts(contexts, m)
    return _roll(pred, actions.reshape((G * m,) + actions.shape[2:]), goal)


def roll_single(pred, ctx, actions, goal):
    pred._ctx_key = None
    with torch.cuda.device(pred.device):
        pred._set_context(ctx)
    return _roll(pred, actions, goal)


def group_scores(pred, goals, finalweight=10., task_weights=None, n=None, expect=0):
    """``vf_group_pixel_scores`` of the last rollout -> (return code, scores [B], per_task [B, tasks])."""
    ntask = pred.n_cam * pred.cfg.ndesig
    n = n or 1
    with torch.cuda.device(pred.device):
        goal_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(goals).reshape(-1), dtype=np.int32)).to(pred.device)
        scores = torch.zeros(n, dtype=torch.float64, device=pred.device)
        per_task = torch.zeros((n, max(ntask, 1)), dtype=torch.float64, device=pred.device)
        w = None
        if task_weights is not None:
            flat = np.asarray(task_weights, dtype=np.float32).reshape(-1)
            w = (ctypes.c_float * flat.size)(*[float(v) for v in flat])
        rc = pred._libh.vf_group_pixel_scores(pred._handle, goal_dev.data_ptr(), ctypes.c_float(finalweight), w,
                                              scores.data_ptr(), per_task.data_ptr(), pred._stream())
        assert rc == expect, (rc, pred._libh.vf_last_error())
        return rc, scores.cpu().numpy(), per_task.cpu().numpy()


def _problems(H, W, nc, T, nd, G, m, ncam, seed):
    rs = np.random.RandomState(seed)
    contexts = [_context(H, W, nd, ncam, nc, rs) for _ in range(G)]
    actions = rs.normal(0, 0.1, (G, m, T, 4))
    goals = rs.randint(-2, max(H, W) + 2, (G, ncam, max(nd, 1), 2))[:, :, :nd]      # some goals lie off-image
    return contexts, actions, goals


def assert_same_bits(got, want, what=''):
    for name, a, b in zip(('frames', 'distrib', 'states', 'scores', 'per_task'), got, want):
        if a is None and b is None:
            continue
        np.testing.assert_array_equal(a, b, err_msg='%s %s' % (what, name))


def singles(pred, contexts, actions, goal):
    """G single-context rollouts, one per group, stacked on the row axis as the grouped rollout lays its rows out."""
    parts = [roll_single(pred, contexts[g], actions[g], goal) for g in range(len(contexts))]
    return tuple(None if parts[0][i] is None else np.concatenate([p[i] for p in parts]) for i in range(5))


# (H, W, n_context, T, ndesig, G, m, ncam)
FIRST = (32, 32, 2, 3, 1, 3, 7, 1)
CASES = [FIRST, (40, 56, 1, 2, 2, 2, 8, 1), (48, 64, 3, 2, 1, 5, 1, 1), (32, 32, 2, 2, 0, 2, 3, 1), (32, 32, 2, 2, 1, 2, 3, 2)]


# ------------------------------------------------------------------ 1. bit identity of the rollout
@pytest.mark.parametrize('H,W,nc,T,nd,G,m,ncam', CASES)
def test_grouped_rollout_is_the_single_context_rollouts(H, W, nc, T, nd, G, m, ncam):
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc, ncam=ncam)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=H + W + G + m)
    goal = goals[0] if nd else None
    got = roll_grouped(pred, contexts, actions, goal)
    assert got[0].shape[0] == G * m
    assert_same_bits(got, singles(pred, contexts, actions, goal))
    # the groups are different problems: a row of group 1 is not the row group 0's context gives the same actions
    other = roll_single(pred, contexts[0], actions[1], goal)
    assert not np.array_equal(other[0], got[0][m:2 * m])


@pytest.mark.parametrize('extra', [dict(decoder='public'), dict(transformation='flow'), dict(transformation='dna'),
                                   dict(transformation='stp'), dict(precision='bf16x6'), dict(precision='bf16')],
                         ids=['layer_spec1', 'layer_spec2', 'layer_spec3', 'layer_spec4', 'precision1', 'precision2'])
def test_every_compositing_table_and_precision(extra):
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc, **extra)
    want_spec = {'public': 1}.get(extra.get('decoder'), {'flow': 2, 'dna': 3, 'stp': 4}.get(extra.get('transformation'), 0))
    assert pred._c_cfg.layer_spec == want_spec and pred._c_cfg.arch == 0
    if want_spec == 3:
        assert pred._c_cfg.num_masks == 1
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=77)
    got = roll_grouped(pred, contexts, actions, goals[0])
    assert np.isfinite(got[0]).all() and np.isfinite(got[3]).all()
    assert_same_bits(got, singles(pred, contexts, actions, goals[0]), str(extra))


def test_every_launch_route_gives_the_same_bits():
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=78)
    want = singles(pred, contexts, actions, goals[0])
    routes = [('set_persistent', 0), ('set_persistent', 1), ('set_xcd_queues', 0), ('set_xcd_queues', 1), ('set_fuse_top', 0),
              ('set_fuse_top', 1), ('set_dedup', 0), ('set_dedup', 1)]
    for setter, value in routes:
        getattr(pred, setter)(value)
        assert_same_bits(roll_grouped(pred, contexts, actions, goals[0]), want, '%s(%d)' % (setter, value))
    # both at once: the per-layer launches without de-duplication
    pred.set_persistent(0)
    pred.set_dedup(0)
    assert_same_bits(roll_grouped(pred, contexts, actions, goals[0]), want, 'per-layer, dedup off')
    assert_same_bits(singles(pred, contexts, actions, goals[0]), want, 'singles, per-layer, dedup off')


def test_one_group_is_the_broadcast_mode():
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, 1, G * m, ncam, seed=79)
    assert_same_bits(roll_grouped(pred, contexts, actions, goals[0]), roll_single(pred, contexts[0], actions[0], goals[0]))


def test_the_shared_cache_is_not_left_stale():
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=80)
    before = roll_single(pred, contexts[1], actions[1], goals[1])
    cached = _roll(pred, actions[1], goals[1])              # the same context again: the context-only units are cached
    assert_same_bits(cached, before)
    roll_grouped(pred, contexts, actions, goals[0])
    after = roll_single(pred, contexts[1], actions[1], goals[1])
    assert_same_bits(after, before, 'after a grouped rollout')
    assert_same_bits(_roll(pred, actions[1], goals[1]), before, 'cached, after a grouped rollout')
    # score() finds its context key dropped and uploads again
    s0, _ = pred.score(contexts[1], {'actions': actions[1]}, goals[1])
    pred._set_contexts(contexts, m)
    s1, _ = pred.score(contexts[1], {'actions': actions[1]}, goals[1])
    np.testing.assert_array_equal(s0, before[3])
    np.testing.assert_array_equal(s1, before[3])


# ------------------------------------------------------------------ 2. the grouped cost
@pytest.mark.parametrize('H,W,nc,T,nd,G,m,ncam', CASES[:3])
def test_grouped_cost_is_the_pinned_cost_of_the_exported_distributions(H, W, nc, T, nd, G, m, ncam):
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=H + W + G + m + 1)
    f, d, s, own, own_pt = roll_grouped(pred, contexts, actions, goals[0])
    _, scores, per_task = group_scores(pred, goals, n=G * m)
    rs = np.random.RandomState(4)
    weights = rs.dirichlet(np.ones(ncam * nd), G)
    _, w_scores, w_per_task = group_scores(pred, goals, task_weights=weights, n=G * m)
    for g in range(G):
        rows = slice(g * m, (g + 1) * m)
        want, want_pt = pixel_cost.eval_pixel_cost(d[rows], goals[g], 10.)
        print('group %d: max rel err scores %.3g per task %.3g' % (g, np.abs(scores[rows] / want - 1).max(),
                                                                   np.abs(per_task[rows] / want_pt - 1).max()))
        np.testing.assert_allclose(scores[rows], want, rtol=2e-6)
        np.testing.assert_allclose(per_task[rows], want_pt, rtol=2e-6)
        np.testing.assert_allclose(w_per_task[rows], want_pt, rtol=2e-6)
        np.testing.assert_allclose(w_scores[rows], (want_pt * weights[g][None]).sum(axis=1), rtol=2e-6)
    # group 0's goal is the goal vf_rollout scored every row against
    np.testing.assert_allclose(scores[:m], own[:m], rtol=2e-6)
    np.testing.assert_allclose(per_task[:m], own_pt[:m], rtol=2e-6)
    # another finalweight
    _, s1, _ = group_scores(pred, goals, finalweight=1., n=G * m)
    np.testing.assert_allclose(s1[:m], pixel_cost.eval_pixel_cost(d[:m], goals[0], 1.)[0], rtol=2e-6)

    # a row's cost has the same bits wherever its group lies and whatever G is
    order = [G - 1, 0]
    roll_grouped(pred, [contexts[g] for g in order], actions[order], goals[0])
    _, moved, moved_pt = group_scores(pred, goals[order], n=2 * m)
    for j, g in enumerate(order):
        np.testing.assert_array_equal(moved[j * m:(j + 1) * m], scores[g * m:(g + 1) * m])
        np.testing.assert_array_equal(moved_pt[j * m:(j + 1) * m], per_task[g * m:(g + 1) * m])


def test_a_raised_status_poisons_the_grouped_cost():
    """``vf_debug_poison_status`` raises the status word from the host (no launch is disturbed): every output is NaN until
    ``vf_device_status`` has read it."""
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=81)
    roll_grouped(pred, contexts, actions, goals[0])
    _, good, _ = group_scores(pred, goals, n=G * m)
    _lib.check(pred._libh.vf_debug_poison_status(pred._handle))
    _, scores, per_task = group_scores(pred, goals, n=G * m)
    assert np.isnan(scores).all() and np.isnan(per_task).all()
    assert pred.device_status() == 1 and pred.device_status() == 0
    _, again, _ = group_scores(pred, goals, n=G * m)
    np.testing.assert_array_equal(again, good)


def test_score_batch_is_the_single_scores():
    H, W, nc, T, nd, G, m, ncam = FIRST
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=82)
    scores, per_task = pred.score_batch(contexts, {'actions': actions}, goals)
    assert scores.shape == (G, m) and per_task.shape == (G, m, 1) and scores.dtype == np.float64
    fetched = [pred.fetch_pixel_distributions(g * m + 2) for g in range(G)]
    for g in range(G):
        want, want_pt = pred.score(contexts[g], {'actions': actions[g]}, goals[g])
        np.testing.assert_allclose(scores[g], want, rtol=2e-6)
        np.testing.assert_allclose(per_task[g], want_pt, rtol=2e-6)
        np.testing.assert_array_equal(fetched[g], pred.fetch_pixel_distributions(2))
    with pytest.raises(ValueError, match='run_batch_size'):
        pred.score_batch(contexts + contexts, {'actions': np.concatenate([actions, actions])}, np.concatenate([goals, goals]))


# ------------------------------------------------------------------ 3. against the oracle
def test_grouped_rollout_matches_the_oracle():
    H, W, nc, T, nd, G, m, ncam = 32, 32, 2, 2, 1, 2, 4, 1
    pred, ws = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=83)
    f, d, s, _, _ = roll_grouped(pred, contexts, actions, goals[0])
    _, scores, per_task = group_scores(pred, goals, n=G * m)
    oracle = OracleCdna(ws[0], torch.float32)
    for g in range(G):
        rows = slice(g * m, (g + 1) * m)
        ctx = contexts[g]
        of, od, os_ = oracle.rollout(ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'],
                                     ctx['context_states'], actions[g])
        assert np.abs(f[rows] - of).max() <= 1e-5
        assert (np.abs(d[rows] - od) / od.max(axis=(3, 4), keepdims=True)).max() <= 2e-5
        assert np.abs(s[rows] - os_).max() <= 1e-6
        want, want_pt = pixel_cost.eval_pixel_cost(od, goals[g], 10.)
        np.testing.assert_allclose(scores[rows], want, rtol=1e-5)
        np.testing.assert_allclose(per_task[rows], want_pt, rtol=1e-5)


# ------------------------------------------------------------------ 4. the planner
# Sampler seeds, designated pixels and goals of the planner test.  Random weights move a distribution little, so the scores of
# a planning call lie close together: goals one pixel from the designated pixels and a wide proposal (initial std 3) spread
# them, and these seeds were chosen on the CPU - the same controllers on ``OracleCdna`` with the same weights - so that the
# K-th and (K + 1)-th score of every iteration of both calls differ by more than 3e-4 relative (the test asserts 1e-4 on the
# engine's own stand-alone run).
PLAN_SEEDS = (78, 11, 160)
PLAN_STD = 3.0


def _planner_setup():
    from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import PhiloxGaussianCEMSampler

    class ParityWeightsPredictor(HipVPredEvaluation):
        def restore(self, weights=None):
            return HipVPredEvaluation.restore(self, parity_weights(self.cfg, 3) if weights is None else weights)

    H = W = 32
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}

    def policy(seed, predictor_class, **over):
        pol = dict(predictor_class=predictor_class, verbose=False, sampler=PhiloxGaussianCEMSampler, device_cem=False,
                   nactions=3, repeat=1, num_samples=12, minimum_selection=3, sampler_seed=seed,     # (3 iterations: the default)
                   initial_std=PLAN_STD, initial_std_lift=PLAN_STD, initial_std_rot=PLAN_STD)
        pol.update(over)
        return pol

    def request(g, t):
        rs = np.random.RandomState(200 + g)
        images = rs.randint(0, 256, (4, 1, H, W, 3)).astype(np.uint8)
        states = rs.normal(0, 0.1, (4, 5))
        desig = [[[6, 9]], [[20, 12]], [[15, 25]]][g]
        goal = [[[7, 10]], [[19, 13]], [[15, 24]]][g]
        return dict(t=t, i_tr=0, desig_pix=desig, goal_pix=goal, images=images[:t + 1], state=states[:t + 1])

    return ParityWeightsPredictor, ag, policy, request


@pytest.mark.parametrize('propagation', [False, True])
def test_planner_plans_as_its_controllers_alone(propagation):
    from visual_foresight_amd.policy.cem_controllers import BatchedPixelCostPlanner, PixelCostController
    Predictor, ag, policy, request = _planner_setup()
    over = {'predictor_propagation': True} if propagation else {}
    G, K = 3, 3
    with quiet():
        planner = BatchedPixelCostPlanner(ag, [policy(s, Predictor, **over) for s in PLAN_SEEDS], 0, 1, G)
        engine = planner.predictor
        assert engine.run_batch_size == G * 12 and engine.sequence_length - engine.n_context == 3
        planner.reset()
        batched = []
        planner.act([request(g, 0) for g in range(G)])      # (below start_planning: the action the context will hold)
        for t in (1, 2):
            res = planner.act([request(g, t) for g in range(G)])
            batched.append([(r['actions'].copy(), {k: v.copy() for k, v in r['plan_stat'].items()},
                             planner.controllers[g]._best_indices.copy()) for g, r in enumerate(res)])
        for g in range(G):
            # the same controller alone, on the same engine
            alone = PixelCostController(ag, policy(PLAN_SEEDS[g], lambda *a, **k: engine, **over), 0, 1)
            alone.reset()
            alone.act(**request(g, 0))
            for call, t in enumerate((1, 2)):
                res = alone.act(**request(g, t))
                act_b, stat_b, elites_b = batched[call][g]
                assert sorted(stat_b) == sorted(res['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
                for key, want in res['plan_stat'].items():
                    # the condition under which a 2e-6 difference cannot reorder the elites, on the stand-alone run itself
                    ranked = np.sort(want)
                    gap = (ranked[K] - ranked[K - 1]) / abs(ranked[K - 1])
                    print('problem %d call %d %s: elite gap %.3g, max rel diff %.3g'
                          % (g, call, key, gap, np.abs(stat_b[key] / want - 1).max()))
                    assert gap > 1e-4, (g, call, key, gap)
                    np.testing.assert_allclose(stat_b[key], want, rtol=2e-6)
                    np.testing.assert_array_equal(np.argsort(stat_b[key])[:K], np.argsort(want)[:K])
                np.testing.assert_array_equal(elites_b, alone._best_indices)
                np.testing.assert_array_equal(act_b, res['actions'])


# ------------------------------------------------------------------ 5. refusals
def _refused(pred, rc):
    assert rc == -1, rc                                                    # VF_ERR_INVALID
    msg = pred._libh.vf_last_error().decode()
    assert 'grouped contexts' in msg, msg
    return msg


def _raw_set_contexts(pred, G, rpg, frames=True, states=True, actions=True, distrib=True):
    c, nc = pred.cfg, pred.n_context
    n = max(G, 1)
    with torch.cuda.device(pred.device):
        f = torch.zeros((n, nc, pred.n_cam, c.height, c.width, 3), dtype=torch.uint8, device=pred.device)
        s = torch.zeros((n, nc, c.sdim), dtype=torch.float32, device=pred.device)
        a = torch.zeros((n, max(nc - 1, 1), c.adim), dtype=torch.float32, device=pred.device)
        d = torch.ones((n, nc, pred.n_cam, c.height, c.width, max(c.ndesig, 1)), dtype=torch.float32, device=pred.device)
        rc = pred._libh.vf_set_contexts(pred._handle, G, rpg, f.data_ptr() if frames else None, s.data_ptr() if states else None,
                                        a.data_ptr() if actions else None, d.data_ptr() if distrib else None, pred._stream())
        torch.cuda.synchronize(pred.device)
    return rc


def test_refusals_leave_the_handle_usable():
    H, W, nc, T, nd, G, m, ncam = 32, 32, 2, 2, 1, 2, 3, 1
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=84)
    want = roll_single(pred, contexts[0], actions[0], goals[0])
    # outside grouped mode
    _refused(pred, group_scores(pred, goals, n=G * m, expect=-1)[0])
    for bad in (dict(G=0, rpg=3), dict(G=2, rpg=0), dict(G=-1, rpg=3), dict(G=2, rpg=m + 1), dict(G=2, rpg=3, distrib=False),
                dict(G=2, rpg=3, actions=False), dict(G=2, rpg=3, frames=False)):
        _refused(pred, _raw_set_contexts(pred, **bad))
        assert_same_bits(_roll(pred, actions[0], goals[0]), want, str(bad))         # still in broadcast mode, context intact
    # grouped mode: before a rollout, and a rollout of another B
    pred._set_contexts(contexts, m)
    _refused(pred, group_scores(pred, goals, n=G * m, expect=-1)[0])
    with pytest.raises(_lib.VfError, match='grouped contexts'):
        _roll(pred, actions[0], goals[0])
    got = roll_grouped(pred, contexts, actions, goals[0])
    assert group_scores(pred, goals, n=G * m)[0] == 0
    assert_same_bits([x[:m] for x in got], want)
    with pytest.raises(ValueError, match='run_batch_size'):
        pred._set_contexts(contexts, m + 1)

    # a frames-only handle rolls grouped contexts, takes no distributions and has no grouped pixel cost
    fo, _ = _predictor(H, W, T, 0, bs=G * m, n_context=nc)
    _refused(fo, _raw_set_contexts(fo, G, m, distrib=True))
    assert _raw_set_contexts(fo, G, m, distrib=False) == 0
    ctx_fo, act_fo, _ = _problems(H, W, nc, T, 0, G, m, ncam, seed=85)
    roll_grouped(fo, ctx_fo, act_fo, None)
    _refused(fo, group_scores(fo, np.zeros((G, 1, 1, 2)), n=G * m, expect=-1)[0])
    assert 'frames-only' in fo.score_batch_refusal()
    with pytest.raises(ValueError, match='frames-only'):
        fo.score_batch(ctx_fo, {'actions': act_fo}, np.zeros((G, 1, 0, 2)))


@pytest.mark.parametrize('hp,word', [(dict(arch='savp', image_height=64, image_width=64), 'arch'), (dict(n_draws=2), 'n_draws')])
def test_other_architectures_and_latent_draws_are_refused(hp, word):
    base = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=32, image_width=32, sequence_length=4)
    base.update(hp)
    pred = HipVPredEvaluation('', base)
    msg = _refused(pred, _raw_set_contexts(pred, 2, 2))
    assert word in msg
    assert word in pred.score_batch_refusal()


# ------------------------------------------------------------------ more groups than one launch's weight sets, camera size
def test_more_groups_than_fit_one_launch_of_weights():
    """``task_weights`` travel as launch arguments, 32 groups at a time: 33 groups of one row take two launches of the
    reduction, the second of which scores the last group alone.  Two designated pixels, so the weights matter."""
    H, W, nc, T, nd, G, m, ncam = 32, 32, 2, 2, 2, 33, 1, 1
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=90)
    f, d, s, _, _ = roll_grouped(pred, contexts, actions, goals[0])
    weights = np.random.RandomState(5).dirichlet(np.ones(nd), G)
    assert np.abs(weights[:, 0] - weights[:, 1]).min() > 1e-3
    _, plain, plain_pt = group_scores(pred, goals, n=G)
    _, scores, per_task = group_scores(pred, goals, task_weights=weights, n=G)
    for g in range(G):
        want, want_pt = pixel_cost.eval_pixel_cost(d[g:g + 1], goals[g], 10.)
        np.testing.assert_allclose(plain[g:g + 1], want, rtol=2e-6)
        np.testing.assert_allclose(per_task[g:g + 1], want_pt, rtol=2e-6)
        np.testing.assert_allclose(scores[g:g + 1], (want_pt * weights[g][None]).sum(axis=1), rtol=2e-6)
    np.testing.assert_array_equal(per_task, plain_pt)
    assert not np.allclose(scores, plain, rtol=1e-4)
    # the same through score_batch
    sb, sb_pt = pred.score_batch(contexts, {'actions': actions}, goals, task_weights=weights.reshape(G, 1, nd))
    np.testing.assert_array_equal(sb.reshape(-1), scores)
    np.testing.assert_array_equal(sb_pt.reshape(G, nd), per_task)


def test_camera_size_contexts_are_shrunk_as_the_single_context_is():
    H, W, nc, T, nd, G, m, ncam = 32, 32, 2, 2, 1, 2, 3, 1
    pred, _ = _predictor(H, W, T, nd, bs=G * m, n_context=nc, camera_height=64, camera_width=64)
    assert pred.camera_size == (64, 64)
    contexts, actions, goals = _problems(H, W, nc, T, nd, G, m, ncam, seed=91)
    rs = np.random.RandomState(92)
    for ctx in contexts:
        ctx['context_frames'] = rs.randint(0, 256, (nc + 1, ncam, 64, 64, 3)).astype(np.uint8)
    got = roll_grouped(pred, contexts, actions, goals[0])
    assert_same_bits(got, singles(pred, contexts, actions, goals[0]))
    with pytest.raises(ValueError, match='camera size'):
        pred._set_contexts([dict(contexts[0], context_frames=contexts[0]['context_frames'][:, :, :32, :32])] * G, m)


def test_predictors_that_cannot_roll_grouped_contexts_say_so():
    base = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=32, image_width=32, sequence_length=4)

    class Preparing(HipVPredEvaluation):
        def _prepare(self, context, actions):
            return context, actions

    pred = Preparing('', base)
    assert '_prepare' in pred.grouped_refusal() and '_prepare' in pred.score_batch_refusal()
    with pytest.raises(ValueError, match='_prepare'):
        pred._set_contexts([{}], 1)
    lanes = HipVPredEvaluation('', dict(base, oversubscribe_gpus=1), n_gpus=2)
    assert 'lanes' in lanes.grouped_refusal()
    with pytest.raises(ValueError, match='lanes'):
        lanes.score_batch([{}], {'actions': np.zeros((1, 1, 2, 4))}, np.zeros((1, 1, 1, 2)))
    assert HipVPredEvaluation('', base).score_batch_refusal() is None
