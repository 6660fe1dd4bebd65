"""Device-resident CEM: the kernels of ``csrc/vf_cem.h`` against ``PhiloxGaussianCEMSampler``, a teacher-forced planning call,
``score_device`` against ``score``, and the refusals."""
import contextlib
import io

import numpy as np
import pytest

from tests.helpers import device_cem_cases as cases
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import (
    PhiloxGaussianCEMSampler, select_elites)

MARGIN = 1e-9


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_seeds_keep_clear_of_every_boundary(name):
    """(CPU) no value the twin tests lies within 1e-9 of a rejection limit or of an integer the discretisation floors at:
    an ulp of the device's log / sin / cos cannot flip a decision for these seeds."""
    want = cases.twin_run(name)
    assert want['margin'] > MARGIN
    M, K = cases.CASES[name][:2]
    assert all(c['actions'].shape[0] == M for c in want['calls']) and want['fit_A'].shape[1] == K


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_kernels_match_the_twin(name):
    """Elite indices, trial counts and capped flags equal; mean and A bit for bit; actions within 1 float32 ulp (the free
    steps are the device's float64 log / sin / cos before the final rounding)."""
    assert cases.twin_run(name)['margin'] > MARGIN
    got, want = cases.device_run(name)
    np.testing.assert_array_equal(got['elites'], want['elites'])
    np.testing.assert_array_equal(got['elite_scores'], want['scores'][want['elites']])
    np.testing.assert_array_equal(got['elite_plans'], want['elite_plans'].astype(np.float32))
    assert got['R'] == want['K']
    np.testing.assert_array_equal(got['fit_mean'], want['fit_mean'])
    np.testing.assert_array_equal(got['fit_A'], want['fit_A'])
    differing = total = 0
    for call, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        np.testing.assert_array_equal(g['trials'], w['trials'], err_msg='call %d' % call)
        np.testing.assert_array_equal(g['capped'], w['capped'], err_msg='call %d' % call)
        ulps = cases.ulp_distance(g['actions'], w['actions'].astype(np.float32))
        differing += int((ulps > 0).sum())
        total += ulps.size
        assert ulps.max() <= 1, (call, int(ulps.max()))
    assert sum(int(g['capped'].sum()) for g in got['calls']) == want['n_capped']
    print('%s: %d of %d action values differ from the twin (by one ulp)' % (name, differing, total))
    if name == 'capped':
        assert want['n_capped'] == 3 * want['M']
    if name == 'near_limit':
        assert max(int(c['trials'].max()) for c in want['calls']) > 8


# ----------------------------------------------------------------------------- the planning call
AG = {'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}
POLICY = {'sampler': PhiloxGaussianCEMSampler, 'repeat': 1, 'num_samples': 20, 'verbose': False, 'sampler_seed': 21}
DESIG, GOAL = [[32, 32]], [[16, 48]]


def _inputs():
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, 64, 64, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))
    return frames, states


def _plan(ctrl):
    frames, states = _inputs()
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, desig_pix=DESIG, goal_pix=GOAL, images=frames[:1], state=states[:1])
        return ctrl.act(t=1, i_tr=0, desig_pix=DESIG, goal_pix=GOAL, images=frames, state=states)


@pytest.fixture(scope='module')
def planned():
    """One device-route planning call (64 x 64 CDNA engine, T 5, 20 samples, 3 iterations) with every iteration's candidates
    kept, the contexts its rollouts saw, and what the resident rollout gives afterwards."""
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController(dict(AG), dict(POLICY, predictor_class=HipVPredEvaluation, predictor_propagation=True), 0, 1)
    ctrl.keep_device_candidates = True
    pred = ctrl.predictor
    contexts, inner = [], pred.score_device

    def recording(context, actions_dev, **kw):
        contexts.append({k: np.array(v) for k, v in context.items()})
        return inner(context, actions_dev, **kw)
    pred.score_device = recording
    out = _plan(ctrl)
    del pred.score_device
    shown = ctrl._best_indices[:3]
    rendered = pred.render_plans(shown)
    return dict(ctrl=ctrl, out=out, contexts=contexts, rendered=rendered, shown=shown,
                propagated=np.array(ctrl._chosen_distrib), candidates=ctrl.device_candidates,
                elites=ctrl.device_elite_indices, best_actions=ctrl._best_actions.copy(),
                best_indices=ctrl._best_indices.copy())


@pytest.mark.gpu
def test_planning_call_is_the_teacher_forced_twin(planned):
    """The twin replayed on the device's own scores and candidates, iteration by iteration: every iteration's candidates
    within 1 ulp, the elites, ``_best_actions`` and the action equal.  (A free-running host route is no reference: one ulp in
    an action moves the scores.)"""
    ctrl, out = planned['ctrl'], planned['out']
    assert len(planned['contexts']) == 3 and len(planned['candidates']) == 3
    hp = ctrl._hp
    with contextlib.redirect_stdout(io.StringIO()):
        twin = PhiloxGaussianCEMSampler(hp, 4, 5)
        assert twin.key == ctrl._sampler.key
        proposed = twin.sample_initial_actions(1, hp.num_samples, None)
    n_capped = 0
    for itr in range(3):
        assert twin.last_margin > MARGIN
        device = planned['candidates'][itr]
        assert cases.ulp_distance(device, proposed.astype(np.float32)).max() <= 1, itr
        n_capped += int(twin.last_capped.sum())
        scores = out['plan_stat']['scores_itr%d' % itr]
        assert scores.shape == (20,) and scores.dtype == np.float64 and not np.isnan(scores).any()
        elites = select_elites(scores, 10)
        np.testing.assert_array_equal(planned['elites'][itr], elites)
        if itr < 2:
            proposed = twin.sample_next_actions(hp.num_samples, device[elites].astype(np.float64), scores[elites])
    assert sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
    np.testing.assert_array_equal(planned['best_indices'], elites)
    np.testing.assert_array_equal(planned['best_actions'], device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl._sampler.n_capped == n_capped and ctrl._sampler._call == twin._call == 3
    assert ctrl.predictor.device_status() == 0


@pytest.mark.gpu
def test_score_device_is_score_without_the_gather(planned):
    """Bit for bit on the same actions: the planning call's own scores, a chunked call with a ragged last chunk, and
    ``only_take_first_view``."""
    import torch
    pred = planned['ctrl'].predictor
    for itr in range(3):
        host, _ = pred.score(planned['contexts'][itr], {'actions': planned['candidates'][itr]}, GOAL, finalweight=10.)
        np.testing.assert_array_equal(host, planned['out']['plan_stat']['scores_itr%d' % itr])
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    small = HipVPredEvaluation('', dict(designated_pixel_count=2, run_batch_size=8, adim=4, sdim=5, image_height=64,
                                        image_width=64, sequence_length=7), n_gpus=1, first_gpu=0).restore()
    ctx = dict(planned['contexts'][0])
    ctx['context_pixel_distributions'] = np.repeat(ctx['context_pixel_distributions'], 2, axis=-1)
    actions = np.random.RandomState(5).normal(0, 0.1, (19, 5, 4)).astype(np.float32)
    goal = [[[16, 48], [40, 8]]]
    for first_view in (False, True):
        host, host_pt = small.score(ctx, {'actions': actions}, goal, finalweight=10., only_take_first_view=first_view)
        dev = small.score_device(ctx, torch.from_numpy(actions).to(small.device), goal, finalweight=10.,
                                 only_take_first_view=first_view)
        assert dev.is_cuda and dev.dtype == torch.float64
        np.testing.assert_array_equal(dev.cpu().numpy(), host)
        np.testing.assert_array_equal(small.last_per_task_dev.cpu().numpy(), host_pt)
    # the last chunk (16..18) is resident; an earlier sample is rolled again from the device-side actions
    dev_fetch = [small.fetch_pixel_distributions(i) for i in (17, 3)]
    small.score(ctx, {'actions': actions}, goal, finalweight=10.)
    for i, d in zip((17, 3), dev_fetch):
        np.testing.assert_array_equal(d, small.fetch_pixel_distributions(i))
    with pytest.raises(ValueError):
        small.score_device(ctx, torch.from_numpy(actions), goal)            # a host tensor
    with pytest.raises(ValueError):
        small.score_device(ctx, torch.from_numpy(actions[:, :4]).contiguous().to(small.device), goal)


@pytest.mark.gpu
def test_resident_rollout_serves_the_page_and_the_propagation(planned):
    """Plan rendering and the propagation fetch after the device-route call equal those after a host-route ``score`` fed the
    same final candidates."""
    pred = planned['ctrl'].predictor
    pred.score(planned['contexts'][2], {'actions': planned['candidates'][2]}, GOAL, finalweight=10.)
    rendered = pred.render_plans(planned['shown'])
    for key in ('frames', 'distributions'):
        np.testing.assert_array_equal(planned['rendered'][key], rendered[key])
    np.testing.assert_array_equal(planned['propagated'], pred.fetch_pixel_distributions(int(planned['best_indices'][0])))
    assert planned['propagated'].shape == (5, 1, 64, 64, 1) and planned['propagated'].any()


@pytest.mark.gpu
def test_refusals_and_the_host_route():
    import torch
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor
    hp = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=64, image_width=64, sequence_length=5)
    frames, states = _inputs()
    ctx = {'context_frames': frames, 'context_actions': np.zeros((1, 4)), 'context_states': states,
           'context_pixel_distributions': np.zeros((2, 1, 64, 64, 1), np.float32)}
    ctx['context_pixel_distributions'][:, 0, 32, 32, 0] = 1
    actions = torch.zeros((4, 3, 4), dtype=torch.float32, device='cuda:0')
    lanes = HipVPredEvaluation('', dict(hp, oversubscribe_gpus=1), n_gpus=2, first_gpu=0).restore()
    with pytest.raises(ValueError, match='lanes'):
        lanes.score_device(ctx, actions, GOAL)
    del lanes
    frames_only = HipVPredEvaluation('', dict(hp, designated_pixel_count=0), n_gpus=1, first_gpu=0).restore()
    with pytest.raises(ValueError, match='frames-only'):
        frames_only.score_device(dict(ctx, context_pixel_distributions=None), actions, GOAL)
    del frames_only
    stochastic = StochasticHipPredictor('', dict(hp, n_latent=2, image_height=32, image_width=32), n_gpus=1, first_gpu=0)
    with pytest.raises(ValueError, match='prepares its sequences on the host'):
        stochastic.score_device(ctx, actions, GOAL)
    assert stochastic.score_device_refusal()
    del stochastic

    # a controller whose evaluate_rollouts is not PixelCostController's own stays on the host route, with the same sampler
    calls = []

    class Overridden(PixelCostController):
        def evaluate_rollouts(self, actions, cem_itr):
            calls.append(np.array(actions))
            return super(Overridden, self).evaluate_rollouts(actions, cem_itr)

    pol = dict(POLICY, predictor_class=HipVPredEvaluation, iterations=2)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = Overridden(dict(AG), pol, 0, 1)
    ctrl.predictor.score_device = None          # (would raise if the device route were taken)
    out = _plan(ctrl)
    assert len(calls) == 2 and calls[0].dtype == np.float64 and isinstance(ctrl._sampler, PhiloxGaussianCEMSampler)
    np.testing.assert_array_equal(ctrl._best_indices, select_elites(out['plan_stat']['scores_itr1'], 10))
    # the same controller class with device_cem False: host route too
    with contextlib.redirect_stdout(io.StringIO()):
        off = PixelCostController(dict(AG), dict(pol, device_cem=False), 0, 1)
    off.predictor.score_device = None
    again = _plan(off)
    np.testing.assert_array_equal(again['plan_stat']['scores_itr0'], out['plan_stat']['scores_itr0'])
