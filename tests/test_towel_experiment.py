"""The reference's towel-folding experiments (``experiments/sawyer/towel_classifier/hparams.py`` and
``experiments/offline_exp/towel_classifier/hparams.py``) loaded literally, and ``state_append`` on the engine path.

The ``policy`` dicts come from ``tests/golden/folding_sampler.json`` (``tools/make_golden_folding.py`` read them from the
reference's files); the test sets three keys and no more: ``predictor_class`` (a recording stand-in),
``classifier_conf_path`` (the literal value is a file in somebody's home directory; a JSON of scorer settings takes its place)
and ``classifier_restore_path`` (likewise; cleared = seeded random weights)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests.helpers.fake_frames_only_predictor import make_fake_frames_only_predictor_class
from visual_foresight_amd.policy.cem_controllers import GoalImController, PixelCostController
from visual_foresight_amd.policy.cem_controllers.samplers.folding_sampler import FoldingCEMSampler
from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController, NCECostController

NAMED = {'class:FoldingCEMSampler': FoldingCEMSampler}
SET_BY_THE_TEST = ('predictor_class', 'classifier_conf_path', 'classifier_restore_path')
# hyper-parameters the controllers of this project carry on top of the reference's, and ``start_planning``, which the
# constructor raises to the network's context (the fixture's values are taken before the reference's constructor, which
# cannot run without its scorer package, would do the same)
NOT_COMPARED = SET_BY_THE_TEST + ('model_path', 'vpred_batch_size', 'start_planning')
APPENDED = [0.41, 0.25, 0.166]


@contextlib.contextmanager
def _quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


@pytest.fixture(scope='module')
def towel(golden_dir):
    with open(os.path.join(golden_dir, 'folding_sampler.json')) as f:
        return json.load(f)['towel']


def _recording(T, H, W, frames_only=True, cheap=False):
    """The fake frames-only predictor, told the agent's sizes as the engine is, remembering the states it is handed.
    ``cheap``: frames that are constant over the image (one value per candidate and step), made without the blob."""
    base = make_fake_frames_only_predictor_class(T, H, W, frames_only=frames_only)

    class Recording(base):
        wants_agent_params = True

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(Recording, self).__init__(model_path, hparams, n_gpus=n_gpus, first_gpu=first_gpu)
            self.states_seen = []

        def __call__(self, context, inputs):
            self.states_seen.append(context['context_states'])
            if not cheap:
                return super(Recording, self).__call__(context, inputs)
            actions = np.asarray(inputs['actions'], dtype=np.float64)
            self.actions_seen.append(actions.copy())
            value = (0.5 + 0.1 * np.tanh(np.cumsum(actions[:, :, :3].sum(axis=-1), axis=1))).astype(np.float32)
            frames = np.broadcast_to(value[:, :, None, None, None, None], actions.shape[:2] + (1, H, W, 3))
            return {'predicted_frames': frames, 'predicted_pixel_distributions': None}

    return Recording


class _CornerScored(ClassifierController):
    """Scores the 600 x 15 frames of the offline experiment by one pixel each instead of the CPU scorer network."""
    def _host_scores(self, gen_images, goal_enc):
        self.cost_perstep = np.asarray(gen_images[:, :, 0, 0, 0, 0], dtype=np.float64)
        return self._weight_scores(self.cost_perstep)


@pytest.mark.parametrize('name,M', [('sawyer', 18), ('offline', 600)])
def test_the_towel_policy_dict_loads_literally_and_plans(towel, name, M, tmp_path):
    case = towel[name]
    assert case['controller'] == 'ClassifierController' and case['policy']['num_samples'] == M
    assert case['conf']['sdim'] == 8 and case['conf']['adim'] == 4 and case['conf']['model'] == 'appflow'
    H, W = case['agent']['image_height'], case['agent']['image_width']
    assert (H, W) == (48, 64) == tuple(case['conf']['orig_size'])
    pdict = {k: NAMED.get(v, v) if isinstance(v, str) else v for k, v in case['policy'].items()}
    assert not any(isinstance(v, str) and v.startswith('class:') for v in pdict.values())
    assert pdict['sampler'] is FoldingCEMSampler and pdict['state_append'] == APPENDED
    conf = str(tmp_path / 'scorer.json')
    with open(conf, 'w') as f:
        json.dump({'seed': 5, 'bias_scale': 0.2}, f)
    pdict['predictor_class'] = _recording(15, H, W, cheap=M > 18)
    pdict['classifier_conf_path'] = conf
    del pdict['classifier_restore_path']
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    with _quiet():
        ctrl = (ClassifierController if M == 18 else _CornerScored)(dict(ag), pdict, 0, 1)
    vals = ctrl._hp.values()
    want = case['values']
    for k, v in want.items():
        if k == 'sampler':
            assert 'class:' + vals[k].__name__ == v
        elif k not in NOT_COMPARED:
            assert vals[k] == v, (k, vals[k], v)
    assert set(vals) - set(NOT_COMPARED) == set(want) - set(NOT_COMPARED)
    assert set(want) <= set(vals)
    assert ctrl._hp.start_planning == ctrl.predictor.n_context - 1 == 1 and want['start_planning'] == 0
    # the predictor is built for the agent's five state dimensions plus the three appended constants
    assert ctrl.predictor.hparams['sdim'] == 8 == case['conf']['sdim'] and ctrl._sdim == 5
    assert ctrl.predictor.hparams['adim'] == 4 and ctrl.predictor.hparams['sequence_length'] == 15 + 2
    assert ctrl.predictor.frames_only and ctrl._elite_count() == (10 if M == 18 else 30)

    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    with _quiet():
        ctrl.reset()
        np.random.seed(0)
        first = ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1])
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states)
    np.testing.assert_array_equal(first['actions'], np.zeros(4))
    pred = ctrl.predictor
    assert len(pred.actions_seen) == len(pred.states_seen) == 3                      # one call per CEM iteration
    for actions, seen in zip(pred.actions_seen, pred.states_seen):
        assert actions.shape == (M, 15, 4)
        assert seen.shape == (2, 8)
        np.testing.assert_array_equal(seen[:, :5], states)
        np.testing.assert_array_equal(seen[:, 5:], np.tile(APPENDED, (2, 1)))
    # the sampler got the agent's own state
    assert ctrl._sampler.b_sdim == 5
    np.testing.assert_array_equal(ctrl._sampler._current_state, states[-1, :2])
    assert np.abs(pred.actions_seen[0][:, :, 2]).max() == 1. / 3                       # the scripted lifts, clipped
    for itr in range(3):
        s = out['plan_stat']['scores_itr%d' % itr]
        assert s.shape == (M,) and np.isfinite(s).all() and len(np.unique(s)) > M // 2
    assert out['actions'].shape == (4,) and ctrl._t_since_replan == 0


# ---------------------------------------------------------------------------------------- state_append, four controllers
AG = {'adim': 4, 'sdim': 5, 'image_height': 16, 'image_width': 32}
CONTROLLERS = {'pixel_cost': PixelCostController, 'goal_image': GoalImController, 'classifier': ClassifierController,
               'nce': NCECostController}


def _plan(kind, **over):
    T, H, W = 4, AG['image_height'], AG['image_width']
    pol = dict(repeat=1, rejection_sampling=False, num_samples=12, iterations=2, nactions=T, verbose=False,
               predictor_class=_recording(T, H, W, frames_only=False), **over)
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal = rs.uniform(0, 1, (1, 1, H, W, 3)).astype(np.float32)
    kw = {'pixel_cost': {'desig_pix': [[8, 8]], 'goal_pix': [[3, 12]]}, 'classifier': {}, 'nce': {'goal_image': goal},
          'goal_image': {'goal_image': goal[0]}}[kind]
    with _quiet():
        ctrl = CONTROLLERS[kind](dict(AG), pol, 0, 1)
        ctrl.reset()
        np.random.seed(0)
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states, **kw)
    return ctrl, out, states


@pytest.mark.parametrize('kind', sorted(CONTROLLERS))
def test_without_state_append_the_predictor_sees_the_agents_state_as_before(kind):
    ctrl, out, states = _plan(kind)
    assert ctrl._hp.state_append is None and ctrl.predictor.hparams['sdim'] == 5
    assert len(ctrl.predictor.states_seen) == 2
    assert all(seen is states for seen in ctrl.predictor.states_seen)        # the very buffer, not a copy
    assert all(c['context_states'] == (2, 5) for c in ctrl.predictor.contexts)


@pytest.mark.parametrize('kind', sorted(CONTROLLERS))
def test_state_append_reaches_the_predictor(kind):
    ctrl, out, states = _plan(kind, state_append=[0.5, -1.0])
    assert ctrl.predictor.hparams['sdim'] == 7 and ctrl._sdim == 5
    assert len(ctrl.predictor.states_seen) == 2
    for seen in ctrl.predictor.states_seen:
        assert seen.shape == (2, 7) and seen.dtype == states.dtype
        np.testing.assert_array_equal(seen[:, :5], states)
        np.testing.assert_array_equal(seen[:, 5:], [[0.5, -1.0], [0.5, -1.0]])
    plain, plain_out, _ = _plan(kind)
    np.testing.assert_array_equal(out['actions'], plain_out['actions'])       # the fake's frames do not read the state
    assert plain._sampler.b_sdim == ctrl._sampler.b_sdim == 5


def test_context_states_are_those_of_the_legacy_boundary(golden_dir):
    """``pred_util.get_context`` is pinned by ``tests/golden/pred_util.npz`` with ``state_append`` [0.5, -1.0]: the engine
    path's helper hands the predictor the same rows."""
    import types
    from visual_foresight_amd.hparams import HParams
    from visual_foresight_amd.policy.cem_controllers.pixel_cost_controller import context_states
    g = np.load(os.path.join(golden_dir, 'pred_util.npz'))
    state = g['ctx/state']
    ctrl = types.SimpleNamespace(_hp=HParams(state_append=None), _state=state[:5])
    assert context_states(ctrl) is ctrl._state
    ctrl._hp.state_append = [0.5, -1.0]
    got = context_states(ctrl)
    np.testing.assert_array_equal(got[-2:][None], g['ctx/states_out'])
    assert got.shape == (5, 5) and got.dtype == g['ctx/states_out'].dtype
