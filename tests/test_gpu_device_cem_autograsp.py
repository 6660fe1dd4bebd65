"""Device-resident CEM for the autograsp sampler: ``cem_sample_autograsp_kernel`` and ``cem_grip_share_kernel`` (with
``cem_refit_kernel`` as their refit) of ``csrc/vf_cem.h`` against ``PhiloxAutograspSampler``; a teacher-forced planning call by
height and by the elites' share; the refusals."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from tests.helpers import device_cem_autograsp_cases as cases
from visual_foresight_amd.policy.cem_controllers.samplers import philox_autograsp_sampler as pas
from visual_foresight_amd.policy.cem_controllers.samplers.philox_autograsp_sampler import PhiloxAutograspSampler
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import select_elites

MARGIN = 1e-9


def lift_bound(hp, T, moves32):
    """What one float32 ulp per step can move a height: ``T * action_norm_factor * 2**-23 * max|lift|``."""
    return T * hp.action_norm_factor * 2.0 ** -23 * float(np.abs(moves32[:, :, pas.LIFT]).max())


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_kernels_match_the_twin(name):
    """Elite indices, scores and plans, ``R``, ``mean`` and ``A`` bit for bit (the refit is ``vf_cem_refit``); trials and capped
    flags equal; moves within 1 float32 ulp (the free steps are the device's float64 log / sin / cos before the final
    rounding).  The gripper column of every device call equals the specification applied to the DEVICE'S OWN float32 moves
    (or to the share of the device's own elites) bit for bit, whatever the ulps do; it equals the twin's column because the
    seeds keep every height clear of ``z_thresh`` (``test_seeds_keep_clear_of_every_boundary``); the tail is exact."""
    got, want = cases.device_run(name)
    s, K, M = want['sampler'], want['K'], want['M']
    hp, n = s._hp, s._adim              # n: the move channels; column n is the gripper
    assert want['margin'] > MARGIN
    for refit in range(2):
        np.testing.assert_array_equal(got['elites'][refit], want['elites'][refit])
        np.testing.assert_array_equal(got['elite_scores'][refit], want['scores'][refit][want['elites'][refit]])
        np.testing.assert_array_equal(got['elite_plans'][refit], want['elite_plans'][refit].astype(np.float32))
        assert got['R'][refit] == K
        np.testing.assert_array_equal(got['fit_mean'][refit], want['fit_mean'][refit])
        np.testing.assert_array_equal(got['fit_A'][refit], want['fit_A'][refit])
    differing = total = grip_differing = 0
    for call, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        assert g.shape == w.shape and g.dtype == np.float32 and np.isfinite(g).all()
        T = g.shape[1]
        np.testing.assert_array_equal(got['trials'][call], want['trials'][call], err_msg='call %d' % call)
        np.testing.assert_array_equal(got['capped'][call], want['capped'][call], err_msg='call %d' % call)
        ulps = cases.ulp_distance(g[:, :, :n], w[:, :, :n].astype(np.float32))
        differing += int((ulps > 0).sum())
        total += ulps.size
        assert ulps.max() <= 1, (call, int(ulps.max()))
        if s.by_share(call):
            share = pas.elite_share(got['elite_plans'][call - 1], hp, n)
            np.testing.assert_array_equal(got['share'][call], share, err_msg='share, call %d' % call)
            np.testing.assert_array_equal(share, want['share'][call])
            own = pas.gripper_from_share(got['share'][call], hp, s.key, call, np.arange(M))
        else:
            assert want['grip_margin'][call] > lift_bound(hp, T, g), call
            own = pas.gripper_from_moves(np.ascontiguousarray(g[:, :, :n]), s.state_z(), hp, s.key, call, np.arange(M))
        np.testing.assert_array_equal(g[:, :, n], own, err_msg='gripper of the device moves, call %d' % call)
        grip_differing += int((g[:, :, n] != w[:, :, n].astype(np.float32)).sum())
        np.testing.assert_array_equal(g[:, :, n + 1:], w[:, :, n + 1:].astype(np.float32), err_msg='tail, call %d' % call)
    print('%s: %d of %d move values differ from the twin (by one ulp), %d gripper values' % (name, differing, total, grip_differing))
    assert grip_differing == 0
    assert sum(int(c.sum()) for c in got['capped']) == want['n_capped']
    if name == 'capped':
        assert want['n_capped'] == 3 * M


@pytest.mark.gpu
def test_refusals_launch_nothing():
    import torch
    from visual_foresight_amd import _lib
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceAutograspCEM, autograsp_config, grip_config
    s = cases.twin_run('latch')['sampler']
    dc = DeviceAutograspCEM(s, 10, 1, 40, 'cuda:0')
    dc.actions.fill_(7.0)
    lib = _lib.load_library()
    ptr = dict(workspace=dc.workspace.data_ptr(), elite_plans=dc.elite_plans.data_ptr(), share=dc.share.data_ptr(),
               actions=dc.actions.data_ptr(), trials=dc.trials.data_ptr(), capped=dc.capped.data_ptr())

    def launch(cfg=None, grip=None, M=40, **over):
        cfg = autograsp_config(s, 10) if cfg is None else cfg
        grip = grip_config(s, False) if grip is None else grip
        p = dict(ptr, **over)
        return lib.vf_cem_sample_autograsp(0, ctypes.byref(cfg) if cfg != 'null' else None,
                                           ctypes.byref(grip) if grip != 'null' else None, p['workspace'], 0, M,
                                           p['elite_plans'], p['share'], p['actions'], p['trials'], p['capped'], None)

    def refused(**kw):
        assert launch(**kw) == -1, kw
        assert b'vf_cem_sample_autograsp' in lib.vf_last_error(), lib.vf_last_error()

    refused(cfg='null')
    refused(grip='null')
    for name in ('workspace', 'actions', 'trials', 'capped'):
        refused(**{name: None})                                                 # a NULL pointer
    refused(workspace=ptr['workspace'] + 8)                                     # misaligned
    for name in ('actions', 'trials', 'capped'):
        refused(**{name: ptr[name] + 2})
    # an invalid move config, fewer than 3 move channels, a row wider than 8, no room for the gripper column
    for change in (dict(nactions=0), dict(repeat=0), dict(n_elites=1), dict(max_trials=0), dict(nactions=43), dict(adim=2),
                   dict(tail=6), dict(tail=0)):
        cfg = autograsp_config(s, 10)
        for k, v in change.items():
            setattr(cfg, k, v)
        refused(cfg=cfg)
    for M in (0, 4097):
        refused(M=M)
    for change in (dict(deviation_prob=-0.1), dict(deviation_prob=1.5), dict(deviation_prob=float('nan')), dict(mode=2)):
        grip = grip_config(s, False)
        for k, v in change.items():
            setattr(grip, k, v)
        refused(grip=grip)
    refused(grip=grip_config(s, True), elite_plans=None)                        # share mode without elite plans or scratch
    refused(grip=grip_config(s, True), share=None)
    refused(grip=grip_config(s, True), share=ptr['share'] + 2)
    torch.cuda.synchronize()
    assert (dc.actions == 7.0).all()
    assert launch(elite_plans=None, share=None) == 0                            # height mode reads neither
    torch.cuda.synchronize()
    assert not (dc.actions[0] == 7.0).any()


# ----------------------------------------------------------------------------- the planning call
AG = {'adim': 4, 'sdim': 5, 'image_height': 64, 'image_width': 64}
POLICY = {'sampler': PhiloxAutograspSampler, 'repeat': 1, 'num_samples': 20, 'verbose': False, 'sampler_seed': 23}
DESIG, GOAL = [[32, 32]], [[16, 48]]


def _inputs():
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, 64, 64, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))
    states[:, 2] = 0.25                 # a height from which five lift steps end on either side of z_thresh
    return frames, states


def _plan(ctrl):
    frames, states = _inputs()
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, desig_pix=DESIG, goal_pix=GOAL, images=frames[:1], state=states[:1])
        return ctrl.act(t=1, i_tr=0, desig_pix=DESIG, goal_pix=GOAL, images=frames, state=states)


@pytest.mark.gpu
@pytest.mark.parametrize('no_refit', [True, False])
def test_planning_call_is_the_teacher_forced_twin(no_refit):
    """One device-route planning call (64 x 64 CDNA engine, T 5, 20 samples, 3 iterations) against the twin replayed on the
    device's own scores and candidates, iteration by iteration: every iteration's moves within 1 ulp and its gripper column
    equal, the elites, ``_best_actions`` and the action equal.  By height throughout (``no_refit``) and by the elites' share
    from the second iteration on."""
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceAutograspCEM
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    pol = dict(POLICY, predictor_class=HipVPredEvaluation) if no_refit else dict(POLICY, predictor_class=HipVPredEvaluation,
                                                                                 no_refit=False)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController(dict(AG), pol, 0, 1)
    ctrl.keep_device_candidates = True
    out = _plan(ctrl)
    assert type(ctrl._device_cem) is DeviceAutograspCEM and len(ctrl.device_candidates) == 3
    hp = ctrl._hp
    _, states = _inputs()
    with contextlib.redirect_stdout(io.StringIO()):
        twin = PhiloxAutograspSampler(hp, 4, 5)
        assert twin.key == ctrl._sampler.key
        proposed = twin.sample_initial_actions(1, hp.num_samples, states[-1])
    n_capped, seen = 0, set()
    for itr in range(3):
        device = ctrl.device_candidates[itr]
        assert device.shape == (20, 5, 4) and device.dtype == np.float32
        assert twin.last_margin > MARGIN
        if not twin.by_share(itr):
            assert twin.last_grip_margin > lift_bound(hp, 5, device), itr
        assert cases.ulp_distance(device[:, :, :3], proposed[:, :, :3].astype(np.float32)).max() <= 1, itr
        np.testing.assert_array_equal(device[:, :, 3], proposed[:, :, 3].astype(np.float32), err_msg='gripper, itr %d' % itr)
        seen |= set(np.unique(device[:, :, 3]).tolist())
        n_capped += int(twin.last_capped.sum())
        scores = out['plan_stat']['scores_itr%d' % itr]
        assert scores.shape == (20,) and scores.dtype == np.float64 and not np.isnan(scores).any()
        elites = select_elites(scores, 10)
        np.testing.assert_array_equal(ctrl.device_elite_indices[itr], elites)
        if itr < 2:
            proposed = twin.sample_next_actions(hp.num_samples, device[elites].astype(np.float64), scores[elites])
    assert seen == {-1.0, 1.0}
    assert sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
    np.testing.assert_array_equal(ctrl._best_indices, elites)
    np.testing.assert_array_equal(ctrl._best_actions, device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl._sampler.n_capped == n_capped and ctrl._sampler._call == twin._call == 3
    np.testing.assert_array_equal(ctrl._sampler.last_trials, twin.last_trials)
    assert ctrl.predictor.device_status() == 0


@pytest.mark.gpu
def test_every_refusal_runs_the_same_sampler_on_the_host_route():
    """``device_cem`` False is the host route by definition; in-process lanes and an overridden ``evaluate_rollouts`` return
    exactly what it returns."""
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation

    class Lanes(HipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(Lanes, self).__init__(model_path, dict(hparams, oversubscribe_gpus=1), n_gpus=2, first_gpu=first_gpu)

    calls = []

    class Overridden(PixelCostController):
        def evaluate_rollouts(self, actions, cem_itr):
            calls.append(np.array(actions))
            return super(Overridden, self).evaluate_rollouts(actions, cem_itr)

    pol = dict(POLICY, predictor_class=HipVPredEvaluation, iterations=2, no_refit=False)

    def host_route(ctrl_cls, policy):
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = ctrl_cls(dict(AG), policy, 0, 1)
        ctrl.predictor.score_device = None          # (would raise if the device route were taken)
        out = _plan(ctrl)
        assert getattr(ctrl, '_device_cem', None) is None and ctrl._sampler._call == 2
        assert isinstance(ctrl._sampler, PhiloxAutograspSampler)
        return ctrl, out

    base, want = host_route(PixelCostController, dict(pol, device_cem=False))
    np.testing.assert_array_equal(base._best_indices, select_elites(want['plan_stat']['scores_itr1'], 10))
    assert base._best_actions.shape == (10, 5, 4) and set(np.unique(base._best_actions[:, :, 3])) <= {-1.0, 1.0}
    assert want['actions'].shape == (4,)
    for ctrl_cls, policy in ((Overridden, pol), (PixelCostController, dict(pol, predictor_class=Lanes))):
        ctrl, out = host_route(ctrl_cls, policy)
        for itr in range(2):
            np.testing.assert_array_equal(out['plan_stat']['scores_itr%d' % itr], want['plan_stat']['scores_itr%d' % itr])
        np.testing.assert_array_equal(out['actions'], want['actions'])
        np.testing.assert_array_equal(ctrl._best_actions, base._best_actions)
    assert len(calls) == 2 and calls[0].dtype == np.float64 and calls[0].shape == (20, 5, 4)
    del ctrl.predictor.score_device                 # (the last one has lanes)
    assert 'lanes' in ctrl.predictor.score_device_refusal()
