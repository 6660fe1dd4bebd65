"""Device-resident CEM for the frame-cost planners: ``score_goal_image_device`` / ``score_frames_device`` against the host
entries, one teacher-forced planning call of ``GoalImController``, ``ClassifierController`` and ``NCECostController`` (the
Philox Gaussian sampler, and the folding sampler on a frames-only engine), which route a controller takes, and the towel
``policy`` dict with only its sampler swapped."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.helpers import device_cem_cases as gaussian_cases                                        # noqa: E402
from tests.helpers import device_cem_fold_cases as fold_cases                                       # noqa: E402
from tests.helpers.fake_frames_only_predictor import assert_same_messages                           # noqa: E402
from visual_foresight_amd.policy.cem_controllers import GoalImController                            # noqa: E402
from visual_foresight_amd.policy.cem_controllers.samplers import (PhiloxFoldingCEMSampler,         # noqa: E402
                                                                   PhiloxGaussianCEMSampler)
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import select_elites     # noqa: E402
from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController, NCECostController   # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation, HipVPredEvaluation  # noqa: E402

H = W = 64
T = 5
AG = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
MARGIN = 1e-9       # no tested value of the Gaussian twin this close to a rejection limit (tests/test_gpu_device_cem.py)


def _inputs():
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = np.random.RandomState(2).uniform(0, 1, (2, 5))
    goal = rs.uniform(0, 1, (1, 1, H, W, 3)).astype(np.float32)
    return frames, states, goal


class _Worker(object):
    def __init__(self):
        self.messages = []

    def put(self, message):
        self.messages.append(message)


# ----------------------------------------------------------------------------- 1. the entries
@pytest.mark.parametrize('base', [HipVPredEvaluation, FramesOnlyHipVPredEvaluation])
def test_device_entries_are_the_host_entries_without_the_gather(base):
    """Bit for bit, rows included, on 1, ``run_batch_size`` and ``run_batch_size + 1`` samples (two chunks, a ragged tail)."""
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    bs = 8
    pred = base('', dict(designated_pixel_count=1, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
                         sequence_length=T + 2), n_gpus=1, first_gpu=0).restore()
    assert pred.frames_only == (base is FramesOnlyHipVPredEvaluation) and pred.frame_score_device_refusal() is None
    assert bool(pred.score_device_refusal()) == pred.frames_only
    frames, states, goal = _inputs()
    ctx = {'context_frames': frames, 'context_actions': np.zeros((1, 4)), 'context_states': states}
    shp = dict(image_height=H, image_width=W, ncam=1, max_frames=bs * T, seed=3, bias_scale=0.2)
    classifier = HipFrameScorer('', dict(shp, head='classifier'), pred.device).restore()
    embedding = HipFrameScorer('', dict(shp, head='embedding'), pred.device).restore()
    goal_enc = embedding.goal_enc(goal[0], frames[-1].astype(np.float32) / 255.)
    for M in (1, bs, bs + 1):
        actions = np.random.RandomState(M).normal(0, 0.1, (M, T, 4)).astype(np.float32)
        dev = torch.from_numpy(actions).to(pred.device)
        for steps in ('last', 'weighted'):
            s, pv = pred.score_goal_image(ctx, {'actions': actions}, goal[0], steps=steps, finalweight=7.)
            cps = pred.last_goal_cost_per_step
            got = pred.score_goal_image_device(ctx, dev, goal[0], steps=steps, finalweight=7.)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (M,)
            np.testing.assert_array_equal(got.cpu().numpy(), s)
            rows = pred.last_goal_rows_dev.cpu().numpy()
            assert rows.shape == (M, 2 + T)
            for a, b in zip(pred.split_goal_rows(rows), (s, pv, cps)):
                np.testing.assert_array_equal(a, b)
            assert pred._last_M == (M if M <= bs else M - bs)               # the last chunk is the resident one
        for scorer, enc in ((classifier, None), (embedding, goal_enc)):
            s = pred.score_frames(ctx, {'actions': actions}, scorer, goal_enc=enc, finalweight=50.)
            cps = pred.last_frame_cost_per_step
            got = pred.score_frames_device(ctx, dev, scorer, goal_enc=enc, finalweight=50.)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (M,)
            np.testing.assert_array_equal(got.cpu().numpy(), s)
            rows = pred.last_frame_rows_dev.cpu().numpy()
            np.testing.assert_array_equal(rows[:, 0], s)
            np.testing.assert_array_equal(rows[:, 1:], cps)
            assert len(np.unique(s)) == M
    # the same argument checks
    with pytest.raises(ValueError):
        pred.score_goal_image_device(ctx, dev, goal[0], steps='first')
    with pytest.raises(ValueError):
        pred.score_goal_image_device(ctx, dev, goal[0][:, :32])
    with pytest.raises(ValueError):
        pred.score_goal_image_device(ctx, torch.from_numpy(actions), goal[0])              # a host tensor
    with pytest.raises(ValueError):
        pred.score_frames_device(ctx, dev, embedding)                                       # no goal_enc
    with pytest.raises(ValueError):
        pred.score_frames_device(ctx, dev[:, :4].contiguous(), classifier)
    assert pred.device_status() == 0


# ----------------------------------------------------------------------------- 2. planning calls
GAUSS = {'sampler': PhiloxGaussianCEMSampler, 'repeat': 1, 'num_samples': 20, 'sampler_seed': 21}
FOLD = dict(fold_cases.TOWEL_STD, sampler=PhiloxFoldingCEMSampler, repeat=1, num_samples=18, sampler_seed=22)
# kind -> (controller, predictor class, policy, name of the device entry)
KINDS = {
    'goal_last': (GoalImController, HipVPredEvaluation, dict(GAUSS), 'score_goal_image_device'),
    'goal_weighted': (GoalImController, HipVPredEvaluation, dict(GAUSS, goal_cost_steps='weighted', finalweight=4.),
                      'score_goal_image_device'),
    'classifier': (ClassifierController, HipVPredEvaluation, dict(GAUSS), 'score_frames_device'),
    'nce': (NCECostController, HipVPredEvaluation, dict(GAUSS), 'score_frames_device'),
    'classifier_folding': (ClassifierController, FramesOnlyHipVPredEvaluation, dict(FOLD), 'score_frames_device'),
}


def _act_kwargs(cls, goal):
    return {GoalImController: {'goal_image': goal[0]}, NCECostController: {'goal_image': goal}}.get(cls, {})


def _plan(ctrl, worker=None, record=None):
    """``reset`` and two ``act`` calls (the second plans) -> (out, the contexts the recorded entry saw)."""
    frames, states, goal = _inputs()
    kw = _act_kwargs(_base_of(ctrl), goal)
    contexts = []
    if record:
        inner = getattr(ctrl.predictor, record)

        def recording(context, actions_dev, *args, **kwargs):
            contexts.append({k: np.array(v) for k, v in context.items()})
            return inner(context, actions_dev, *args, **kwargs)
        setattr(ctrl.predictor, record, recording)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states, verbose_worker=worker, **kw)
    if record:
        delattr(ctrl.predictor, record)
    return out, contexts


def _base_of(ctrl):
    for cls in (GoalImController, NCECostController, ClassifierController):
        if isinstance(ctrl, cls):
            return cls


def _teacher_forced(ctrl, out, n_iter=3):
    """The twin replayed on the device's own scores and float32 candidates, iteration by iteration: the candidates within
    the kernels' tolerance (1 ulp for the Gaussian sampler; the folding kernel's bound), the elites of every iteration,
    ``_best_actions``, the executed action and the keys of ``plan_stat`` equal."""
    hp = ctrl._hp
    M, K = hp.num_samples, ctrl._elite_count()
    _, states, _ = _inputs()
    with contextlib.redirect_stdout(io.StringIO()):
        twin = hp.sampler(hp, 4, 5)
        twin.key = ctrl._sampler.key
        proposed = twin.sample_initial_actions(1, M, states[-1])
    assert len(ctrl.device_candidates) == n_iter
    for itr in range(n_iter):
        device = ctrl.device_candidates[itr]
        assert device.shape == proposed.shape and device.dtype == np.float32
        if isinstance(twin, PhiloxGaussianCEMSampler):
            assert twin.last_margin > MARGIN
            assert gaussian_cases.ulp_distance(device, proposed.astype(np.float32)).max() <= 1, itr
        else:
            excess, _ = fold_cases.action_excess(device, proposed)
            assert excess.max() <= 0.0, itr
        scores = out['plan_stat']['scores_itr%d' % itr]
        assert scores.shape == (M,) and scores.dtype == np.float64 and not np.isnan(scores).any()
        elites = select_elites(scores, K)
        np.testing.assert_array_equal(ctrl.device_elite_indices[itr], elites)
        if itr + 1 < n_iter:
            proposed = twin.sample_next_actions(M, device[elites].astype(np.float64), scores[elites])
    assert sorted(out['plan_stat']) == ['scores_itr%d' % i for i in range(n_iter)]         # as on the host route
    np.testing.assert_array_equal(ctrl._best_indices, elites)
    np.testing.assert_array_equal(ctrl._best_actions, device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl._sampler._call == twin._call == n_iter
    assert ctrl.predictor.device_status() == 0


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_planning_call_is_the_teacher_forced_twin_and_sets_what_the_host_route_sets(kind):
    cls, base, pol, entry = KINDS[kind]
    worker = _Worker()
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = cls(dict(AG), dict(pol, predictor_class=base), 0, 1)
    ctrl.keep_device_candidates = True
    out, contexts = _plan(ctrl, worker, record=entry)
    assert len(contexts) == 3                                       # the device route was taken
    assert type(ctrl._device_cem).__name__ == ('DeviceFoldingCEM' if 'folding' in kind else 'DeviceCEM')
    assert ctrl.predictor.frames_only == (base is FramesOnlyHipVPredEvaluation)
    _teacher_forced(ctrl, out)
    # the last iteration on the host route, on the same candidates: scores, per-step costs (per-view costs), the page
    pred, hp, last = ctrl.predictor, ctrl._hp, ctrl.device_candidates[2]
    device_cps, scores = ctrl.cost_perstep.copy(), out['plan_stat']['scores_itr2']
    if cls is GoalImController:
        host, per_view = pred.score_goal_image(contexts[2], {'actions': last}, ctrl._goal_image, steps=hp.goal_cost_steps,
                                               finalweight=hp.finalweight, first_view_only=hp.only_take_first_view)
        np.testing.assert_array_equal(ctrl.goal_cost_per_view, per_view)
        np.testing.assert_array_equal(device_cps, pred.last_goal_cost_per_step)
        assert device_cps.shape == (hp.num_samples, 1, T)
    else:
        host = pred.score_frames(contexts[2], {'actions': last}, ctrl.scorer, goal_enc=ctrl._goal_enc(),
                                 finalweight=hp.finalweight)
        np.testing.assert_array_equal(device_cps, pred.last_frame_cost_per_step)
        assert device_cps.shape == (hp.num_samples, T)
    np.testing.assert_array_equal(host, scores)
    assert any(m[0] == 'mov' for m in worker.messages)
    again = ctrl._verbose_worker = _Worker()
    ctrl._put_plan_page(2, host, contexts[2], last)
    assert_same_messages(worker.messages, again.messages)


# ----------------------------------------------------------------------------- 3. refusals
class _NoEntries(HipVPredEvaluation):
    """A predictor of before the device entries: the host entries alone."""
    @property
    def score_goal_image_device(self):
        raise AttributeError('score_goal_image_device')

    @property
    def score_frames_device(self):
        raise AttributeError('score_frames_device')


class _Lanes(HipVPredEvaluation):
    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        super(_Lanes, self).__init__(model_path, dict(hparams, oversubscribe_gpus=1), n_gpus=2, first_gpu=first_gpu)


def _overridden(cls, calls):
    class Overridden(cls):
        def evaluate_rollouts(self, actions, cem_itr):
            calls.append(np.array(actions))
            return super(Overridden, self).evaluate_rollouts(actions, cem_itr)
    return Overridden


@pytest.mark.parametrize('kind', ['goal_last', 'classifier_folding'])
def test_every_refusal_runs_the_same_sampler_on_the_host_route(kind):
    """``device_cem`` False is the host route by definition; every refused configuration returns exactly what it returns:
    a predictor without the entry, ``verbose_every_iter`` with a verbose worker, an overridden ``evaluate_rollouts``, in-process lanes."""
    cls, base, pol, entry = KINDS[kind]
    pol = dict(pol, predictor_class=base, iterations=2)

    def host_route(ctrl_cls, policy):
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = ctrl_cls(dict(AG), policy, 0, 1)
        if hasattr(type(ctrl.predictor), entry) and not isinstance(ctrl.predictor, _NoEntries):
            setattr(ctrl.predictor, entry, None)            # (would raise if the device route were taken)
        # (every iteration's page needs its rollout resident: verbose_every_iter refuses when there is a worker to put it on)
        out, _ = _plan(ctrl, worker=_Worker() if policy.get('verbose_every_iter') else None)
        assert getattr(ctrl, '_device_cem', None) is None and ctrl._sampler._call == 2
        assert isinstance(ctrl._sampler, pol['sampler'])
        return ctrl, out

    base_ctrl, want = host_route(cls, dict(pol, device_cem=False))
    np.testing.assert_array_equal(base_ctrl._best_indices, select_elites(want['plan_stat']['scores_itr1'], 10))
    calls = []
    refused = [(cls, dict(pol, verbose_every_iter=True)), (_overridden(cls, calls), pol)]
    if kind == 'goal_last':         # (the frames-only class has no lanes of its own to offer; the refusal is the predictor's)
        refused += [(cls, dict(pol, predictor_class=_NoEntries)), (cls, dict(pol, predictor_class=_Lanes))]
    for ctrl_cls, policy in refused:
        ctrl, out = host_route(ctrl_cls, policy)
        for itr in range(2):
            np.testing.assert_array_equal(out['plan_stat']['scores_itr%d' % itr], want['plan_stat']['scores_itr%d' % itr])
        np.testing.assert_array_equal(out['actions'], want['actions'])
        np.testing.assert_array_equal(ctrl._best_actions, base_ctrl._best_actions)
    assert len(calls) == 2 and calls[0].dtype == np.float64
    if kind == 'goal_last':
        del ctrl.predictor.score_goal_image_device          # (the last one has lanes)
        assert 'lanes' in ctrl.predictor.frame_score_device_refusal()
        with pytest.raises(ValueError, match='lanes'):
            ctrl.predictor.score_goal_image_device({}, torch.zeros((1, T, 4), device='cuda:0'), None)


def test_latent_draws_refuse_the_device_entries():
    from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor
    hp = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=32, image_width=32, sequence_length=5,
              n_latent=2)
    stochastic = StochasticHipPredictor('', hp, n_gpus=1, first_gpu=0)
    assert 'prepares its sequences on the host' in stochastic.frame_score_device_refusal()
    with pytest.raises(ValueError, match='prepares its sequences on the host'):
        stochastic.score_frames_device({}, torch.zeros((4, 3, 4), device='cuda:0'), None)


# ----------------------------------------------------------------------------- 4. the towel dict
def test_the_towel_policy_plans_on_the_device_with_only_the_sampler_swapped(golden_dir, tmp_path):
    """``experiments/sawyer/towel_classifier``'s ``policy`` dict (48 x 64, appearance flow, frames-only, 18 x T15, the three
    ``state_append`` constants) with ``PhiloxFoldingCEMSampler`` for ``FoldingCEMSampler``: the planning call takes the device
    route (the driver, the three calls of ``score_frames_device``, the log line) and matches its teacher-forced twin."""
    from tests import test_gpu_towel_experiment as towel
    pol = towel.towel_policy(golden_dir, str(tmp_path / 'scorer_conf.json'))
    assert set(pol) >= {'sampler', 'state_append', 'num_samples'}
    pol['sampler'] = PhiloxFoldingCEMSampler
    frames, states = towel.observations()
    lines = io.StringIO()
    with contextlib.redirect_stdout(lines):
        ctrl = ClassifierController(dict(towel.AG), dict(pol, predictor_class=towel._flow(FramesOnlyHipVPredEvaluation)), 0, 1)
        ctrl.keep_device_candidates = True
        seen, inner = [], ctrl.predictor.score_frames_device
        ctrl.predictor.score_frames_device = lambda c, a, *args, **kw: (seen.append(tuple(a.shape)), inner(c, a, *args, **kw))[1]
        np.random.seed(0)           # (the sampler draws its Philox key from np.random in reset())
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1])
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states)
    log = lines.getvalue()
    assert pol['verbose_every_iter'] is True and 'starting cem at t1 (device route)...' in log     # (no page is asked for)
    assert [log.count('best scores itr %d: ' % i) for i in range(3)] == [1, 1, 1]
    assert seen == [(towel.M, towel.T, 4)] * 3 and type(ctrl._device_cem).__name__ == 'DeviceFoldingCEM'
    pred = ctrl.predictor
    assert pred.frames_only and pred.cfg.sdim == 8 and pred.cfg.transformation == 'flow' and pred.device_status() == 0
    hp = ctrl._hp
    twin = PhiloxFoldingCEMSampler(hp, 4, 5)
    twin.key = ctrl._sampler.key
    proposed = twin.sample_initial_actions(1, towel.M, states[-1])
    assert np.abs(proposed[:, :, :2]).max() <= 0.2 and np.abs(proposed[:, :, 2]).max() == 1. / 3   # the scripted lifts reach the clip
    for itr in range(3):
        device = ctrl.device_candidates[itr]
        excess, _ = fold_cases.action_excess(device, proposed)
        assert device.shape == (towel.M, towel.T, 4) and excess.max() <= 0.0, itr
        scores = out['plan_stat']['scores_itr%d' % itr]
        elites = select_elites(scores, towel.K)
        np.testing.assert_array_equal(ctrl.device_elite_indices[itr], elites)
        assert scores.shape == (towel.M,) and not np.isnan(scores).any()
        if itr < 2:
            proposed = twin.sample_next_actions(towel.M, device[elites].astype(np.float64), scores[elites])
    np.testing.assert_array_equal(ctrl._best_indices, elites)
    np.testing.assert_array_equal(ctrl._best_actions, device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl.cost_perstep.shape == (towel.M, towel.T)
