"""Inverse-model policy: a network emits the next actions from the current image, a goal image and a short context.

API-compatible with the reference's ``visual_mpc/policy/inverse_models/inverse_model_base_controller.py`` (class
``InvModelBaseController`` :6; hyper-parameter defaults :39-57; ``reset`` :59-64; ``act`` :69-94; ``update_context`` :96-102;
``convert_to_float`` :104-106) - same constructor, hyper-parameter names and defaults, and the same host logic step by
step: random context actions ``np.random.uniform(low, high) * context_action_weight`` while ``t < num_context``, a new
plan whenever ``(t - num_context) % replan_every == 0``, ``action_counter`` steps into the plan since, the assertion (with
its text) when a plan runs out, the goal passed on as it comes, images converted with a float64 ``/ 255.``, and ``plan_stat``
created by ``reset()`` only (pinned by tests/test_inverse_model.py against traces of the reference itself).

Departures:

* the default ``predictor_class`` is ``HipActionInference`` (``video_prediction/inverse_model.py``) - the reference's
  ``robonet.inverse_model.testing.action_inference_interface.ActionInferenceInterface`` is not part of the snapshot;
* the predictor's hparams are filled from ``ag_params`` and the policy's own parameters (``adim``, ``image_height``,
  ``image_width``, ``n_context = num_context``, ``n_actions = T``) where the reference passes an empty dict.  They matter
  only while ``model_params_path`` is empty (seeded random weights of that size); a model directory carries its own.
"""
import numpy as np

from visual_foresight_amd.policy.policy import Policy
from visual_foresight_amd.utils.logger import Logger


def _default_predictor_class():
    from visual_foresight_amd.video_prediction.inverse_model import HipActionInference
    return HipActionInference


# (name, default) in registration order (reference :40-52)
INVERSE_MODEL_HPARAMS = (
    ('T', 15),                                      # actions per plan
    ('predictor_class', None),                      # None -> HipActionInference
    ('model_params_path', ''),
    ('model_restore_path', ''),
    ('logging_dir', ''),
    ('load_T', 7),
    ('num_context', 2),
    ('replan_every', 2),
    ('context_action_weight', [1, 1, 1, 1]),
    ('initial_action_low', [-0.025, -0.025, -0.025, 0]),
    ('initial_action_high', [0.025, 0.025, 0.025, 0]),
)

PLAN_EXHAUSTED = ('Tried to take action {} of plan containing {}. '
                  'Maybe re-planning is not occurring often enough?')


def convert_to_float(input):
    """uint8 image -> float64 in [0, 1]."""
    assert input.dtype == np.uint8, "assumed input is uint8"
    return input.astype(np.uint8) / 255.


class InvModelBaseController(Policy):
    def __init__(self, ag_params, policyparams, gpu_id, ngpu):
        self._hp = self._default_hparams()
        self._override_defaults(policyparams)
        self.agentparams = ag_params
        hp = self._hp
        if hp.logging_dir:
            self._logger = Logger(hp.logging_dir, 'cem{}log.txt'.format(ag_params['gpu_id']))
        else:
            self._logger = Logger(printout=True)
        self._logger.log('init inverse model controller')
        self._adim, self._sdim = ag_params['adim'], ag_params['sdim']

        predictor_class = hp.predictor_class if hp.predictor_class is not None else _default_predictor_class()
        predictor_hparams = {'adim': self._adim, 'n_context': hp.num_context, 'n_actions': hp.T}
        predictor_hparams.update({k: ag_params[k] for k in ('image_height', 'image_width') if k in ag_params})
        if 'model_image_height' in ag_params or 'model_image_width' in ag_params:
            # the network is built at the model's size; the camera-size start image, goal image and context frames are
            # shrunk before every inference (video_prediction/resample.py; the reference's agent shrinks its observations)
            from visual_foresight_amd.policy.cem_controllers.pixel_cost_controller import model_image_size
            model = model_image_size(ag_params)
            predictor_hparams.update(image_height=model[0], image_width=model[1],
                                     camera_height=ag_params['image_height'], camera_width=ag_params['image_width'])
        self.predictor = predictor_class(hp.model_params_path, predictor_hparams, n_gpus=ngpu, first_gpu=gpu_id)
        self.predictor.restore()
        self._clear_plan()

    def _default_hparams(self):
        params = super(InvModelBaseController, self)._default_hparams()
        for name, default in INVERSE_MODEL_HPARAMS:
            params.add_hparam(name, default)
        return params

    def _clear_plan(self):
        self.action_counter = 0             # steps taken from the current plan
        self.actions = None                 # the current plan [1, T, adim]
        self.context_actions = [None] * self._hp.num_context
        self.context_frames = [None] * self._hp.num_context

    def reset(self):
        self.plan_stat = {}                 # (exists from the first reset() on, as in the reference)
        self._clear_plan()

    def _sample_initial_action(self):
        return np.random.uniform(self._hp.initial_action_low, self._hp.initial_action_high)

    def _replan(self, images, goal_image):
        """A new plan from the newest frame of camera 0, the goal as it comes, and the context."""
        ctx_frames = np.concatenate([f[None, None] for f in self.context_frames], axis=1)      # [1, num_context, H, W, 3]
        ctx_actions = np.array(self.context_actions)[None]                                      # [1, num_context, adim]
        self.actions = self.predictor(convert_to_float(images[-1, 0]), goal_image[-1, 0], ctx_actions, ctx_frames)
        self.action_counter = 0

    def act(self, t=None, i_tr=None, images=None, goal_image=None):
        hp = self._hp
        if t < hp.num_context:              # no context yet: small random moves
            action = self._sample_initial_action() * hp.context_action_weight
        else:
            if (t - hp.num_context) % hp.replan_every == 0:
                self._replan(images, goal_image)
            print('t {} action counter {}'.format(t, self.action_counter))
            assert self.actions.shape[1] > self.action_counter, \
                PLAN_EXHAUSTED.format(self.action_counter, self.actions.shape[1])
            action = self.actions[0, self.action_counter]
            self.action_counter += 1
        print('action ', action)
        self.update_context(convert_to_float(np.copy(images[-1, 0])), action)
        return {'actions': action, 'plan_stat': self.plan_stat}

    def update_context(self, new_image, new_action):
        """The newest ``num_context`` frames and actions."""
        self.context_frames.append(new_image)
        self.context_actions.append(new_action)
        if len(self.context_frames) > self._hp.num_context:
            del self.context_frames[0], self.context_actions[0]
