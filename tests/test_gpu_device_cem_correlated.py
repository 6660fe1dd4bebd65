"""Device-resident CEM for the correlated-noise sampler: the kernels ``cem_soft_refit_kernel`` / ``cem_sample_corr_kernel``
of ``csrc/vf_cem.h`` against ``PhiloxCorrelatedNoiseSampler``, a teacher-forced planning call, and which route a controller
takes."""
import contextlib
import io

import numpy as np
import pytest

from tests.helpers import device_cem_cases as gaussian_cases
from tests.helpers import device_cem_corr_cases as cases
from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxCorrelatedNoiseSampler, PhiloxGaussianCEMSampler
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import select_elites


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_cases_reach_what_they_name(name):
    """(CPU) the twin's side of every case: shapes, and for ``ties`` that the NaN scores sort last, outside the elites."""
    want = cases.twin_run(name)
    M, K, nactions, adim = cases.CASES[name][:4]
    tail = len(want['tail'] or ())
    assert all(c.shape == (M, nactions, adim + tail) for c in want['calls'])
    assert want['soft'].shape == (K,) and want['soft'][0] == 1.0 and want['centre'].shape == (nactions * adim,)
    assert want['sampler']._call == 3
    if want['sampler']._hp.refit_cov:
        assert want['fit_A'].shape == (nactions * adim, K)
    if name == 'ties':
        assert np.isnan(want['scores']).sum() >= 2 and not np.isnan(want['scores'][want['elites']]).any()
        assert len(set(want['scores'][want['elites']])) < K         # ties inside the elites
    if name == 'smooth_tail':
        assert want['sampler'].first_predecessor().tolist() == [0.03, -0.01, 0.2, -0.4]
        assert (want['calls'][2][:, :, 4:] == np.array([0.25, -1.0])).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_kernels_match_the_twin(name):
    """Elite indices, scores and plans equal; with ``refit_cov`` the plain mean and A bit for bit; ``soft`` within 2 float64
    ulp (``exp`` is within 1 ulp of the true value on each side: ROCm's documented accuracy and glibc's); ``centre`` within
    ``(K + 4) 2^-51 sum_k |e_kd| soft_k / den`` (the 2-ulp perturbation of each ``soft_k`` plus one rounding per
    accumulation step on either side); actions within ``max(1 float32 ulp, 2^-40 max|twin actions of the call|)`` (the
    device's log / sin / cos; the floor is for values the centre or the colouring chains cancel to near zero); the tail
    columns exact."""
    got, want = cases.device_run(name)
    K, adim = want['K'], want['adim']
    np.testing.assert_array_equal(got['elites'], want['elites'])
    np.testing.assert_array_equal(got['elite_scores'], want['scores'][want['elites']])
    np.testing.assert_array_equal(got['elite_plans'], want['elite_plans'].astype(np.float32))
    assert got['valid']
    if want['sampler']._hp.refit_cov:
        assert got['R'] == K
        np.testing.assert_array_equal(got['mean'], want['fit_mean'])
        np.testing.assert_array_equal(got['A'], want['fit_A'])
    else:
        assert got['R'] == 0
    soft_ulps = cases.f64_ulp_distance(got['soft'], want['soft'])
    bound = cases.centre_bound(want['elite_rows'], want['soft'])
    centre_err = np.abs(got['centre'] - want['centre'])
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = np.where(bound > 0, centre_err / bound, np.where(centre_err > 0, np.inf, 0.0))
    print('%s: soft differs by at most %d ulp; centre error at most %.3f of the bound' % (name, soft_ulps.max(), frac.max()))
    differing = total = 0
    worst = []
    for call, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        excess, ulps = cases.action_excess(g[:, :, :adim], w[:, :, :adim])
        differing += int((ulps > 0).sum())
        total += ulps.size
        worst.append(float(excess.max()))
        np.testing.assert_array_equal(g[:, :, adim:], w[:, :, adim:].astype(np.float32), err_msg='tail, call %d' % call)
    print('%s: %d of %d action values differ from the twin at all' % (name, differing, total))
    assert soft_ulps.max() <= 2
    assert (centre_err <= bound).all(), float(frac.max())
    assert max(worst) <= 0.0, worst


# ----------------------------------------------------------------------------- the planning call
AG = {'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}
POLICY = {'sampler': PhiloxCorrelatedNoiseSampler, 'nactions': 5, 'num_samples': 20, 'verbose': False, 'sampler_seed': 21}
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
    """One device-route planning call (64 x 64 CDNA engine, nactions 5, 20 samples, 3 iterations, K 10) with every
    iteration's candidates kept and the contexts its rollouts saw."""
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
    return dict(ctrl=ctrl, out=out, contexts=contexts, propagated=np.array(ctrl._chosen_distrib),
                candidates=ctrl.device_candidates, elites=ctrl.device_elite_indices,
                best_actions=ctrl._best_actions.copy(), best_indices=ctrl._best_indices.copy())


@pytest.mark.gpu
def test_planning_call_is_the_teacher_forced_twin(planned):
    """The twin replayed on the device's own scores and float32 candidates, iteration by iteration: every iteration's
    candidates within the action tolerance, the elites, ``_best_actions`` and the action equal."""
    ctrl, out = planned['ctrl'], planned['out']
    assert type(ctrl._device_cem).__name__ == 'DeviceCorrelatedCEM'
    assert len(planned['contexts']) == 3 and len(planned['candidates']) == 3
    hp = ctrl._hp
    with contextlib.redirect_stdout(io.StringIO()):
        twin = PhiloxCorrelatedNoiseSampler(hp, 4, 5)
        assert twin.key == ctrl._sampler.key
        proposed = twin.sample_initial_actions(1, hp.num_samples, None)
    for itr in range(3):
        device = planned['candidates'][itr]
        assert device.shape == (20, 5, 4) and device.dtype == np.float32
        excess, ulps = cases.action_excess(device, proposed)
        print('iteration %d: %d of %d candidate values differ from the twin at all' % (itr, int((ulps > 0).sum()), ulps.size))
        assert excess.max() <= 0.0, itr
        scores = out['plan_stat']['scores_itr%d' % itr]
        assert scores.shape == (20,) and scores.dtype == np.float64 and not np.isnan(scores).any()
        elites = select_elites(scores, 10)
        np.testing.assert_array_equal(planned['elites'][itr], elites)
        if itr < 2:
            proposed = twin.sample_next_actions(hp.num_samples, device[elites].astype(np.float64), scores[elites])
    assert sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']       # as on the host route
    np.testing.assert_array_equal(planned['best_indices'], elites)
    np.testing.assert_array_equal(planned['best_actions'], device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl._sampler._call == twin._call == 3
    assert ctrl.predictor.device_status() == 0


@pytest.mark.gpu
def test_resident_rollout_serves_the_propagation(planned):
    """The propagated distributions after the device-route call equal those after a host-route ``score`` fed the same final
    candidates."""
    pred = planned['ctrl'].predictor
    host, _ = pred.score(planned['contexts'][2], {'actions': planned['candidates'][2]}, GOAL, finalweight=10.)
    np.testing.assert_array_equal(host, planned['out']['plan_stat']['scores_itr2'])
    np.testing.assert_array_equal(planned['propagated'], pred.fetch_pixel_distributions(int(planned['best_indices'][0])))
    assert planned['propagated'].shape == (5, 1, 64, 64, 1) and planned['propagated'].any()


@pytest.mark.gpu
def test_route_selection():
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
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
    assert len(calls) == 2 and calls[0].dtype == np.float64 and isinstance(ctrl._sampler, PhiloxCorrelatedNoiseSampler)
    np.testing.assert_array_equal(ctrl._best_indices, select_elites(out['plan_stat']['scores_itr1'], 10))
    assert ctrl._sampler._call == 2
    # the same controller class with device_cem False: host route too
    with contextlib.redirect_stdout(io.StringIO()):
        off = PixelCostController(dict(AG), dict(pol, device_cem=False), 0, 1)
    off.predictor.score_device = None
    again = _plan(off)
    np.testing.assert_array_equal(again['plan_stat']['scores_itr0'], out['plan_stat']['scores_itr0'])
    # a PhiloxGaussianCEMSampler controller built in the same process still takes its own route ...
    gauss = dict(pol, sampler=PhiloxGaussianCEMSampler, repeat=1)
    del gauss['nactions']
    with contextlib.redirect_stdout(io.StringIO()):
        g = PixelCostController(dict(AG), gauss, 0, 1)
    g_out = _plan(g)
    assert type(g._device_cem).__name__ == 'DeviceCEM' and g._sampler._call == 2 and g._sampler.last_trials.shape == (20,)
    np.testing.assert_array_equal(g._best_indices, select_elites(g_out['plan_stat']['scores_itr1'], 10))
    # ... and its kernels pass a case of their own helper
    got, want = gaussian_cases.device_run('r_lt_d')
    np.testing.assert_array_equal(got['elites'], want['elites'])
    np.testing.assert_array_equal(got['fit_mean'], want['fit_mean'])
    np.testing.assert_array_equal(got['fit_A'], want['fit_A'])
    for g_call, w_call in zip(got['calls'], want['calls']):
        np.testing.assert_array_equal(g_call['trials'], w_call['trials'])
        assert gaussian_cases.ulp_distance(g_call['actions'], w_call['actions'].astype(np.float32)).max() <= 1
