"""CEM controller scoring rollouts with a learned success classifier.

Restates the reference's ``visual_mpc/policy/cem_controllers/variants/classifier_controller.py`` (ctor :16-55, defaults
:66-81, ``evaluate_rollouts`` :83-133 with the cost at :94-105, ``_weight_scores`` :135-142, ``act`` :145-149) at the same
import path, with the same four-argument constructor, ``act`` signature and hyper-parameters (``finalweight`` 100,
``classifier_conf_path``, ``classifier_restore_path``, ``classifier_batch_size``, ``state_append``, ``compare_to_expert``,
``verbose_img_height``, ``verbose_frac_display``, same defaults) plus the predictor ones the controllers of this project
carry (``predictor_class``, ``model_path``, ``vpred_batch_size``).

Every predicted frame goes through the classifier; the cost of a frame is ``-log(p_success + 1e-5)``, summed over views,
weighted over time by ``_weight_scores``.  With the default predictor (``HipVPredEvaluation``) the frames never leave
the GPU: ``score_frames`` runs a ``HipFrameScorer`` on them where the rollout left them and only score rows come back.
A predictor without ``score_frames`` is scored on the host from the ``predicted_frames`` its ``__call__`` returns, with the
same network (``HostFrameScorer``) and the same arithmetic (``frame_scorer_arch.learned_cost``).

``classifier_restore_path`` is a directory written by ``frame_scorer_arch.save_scorer_weights``; empty = seeded random
weights (as ``model_path=''`` does for the predictor).  ``classifier_conf_path``, if given, is a JSON file of scorer
hyper-parameters (``seed``, ``bias_scale``, ``input_scale``).

Departures from the reference:

(a) The reference puts the scorer on a GPU of its own (``gpu_id + ngpu - 1``, :29-36) and copies every frame to the host and
    back.  Here the scorer runs on every predictor device, because the frames live there.
(b) The network is this project's (``video_prediction/frame_scorer_arch.py``): the reference's ``control_embedding``
    package is not part of the snapshot - PARITY with its networks is UNPINNED; the cost arithmetic around the network is
    pinned by goldens minted from the reference's own code (``tests/golden/learned_cost.*``).
(c) Context actions are the predictor's business here (``context_actions`` of the context dict); the reference's classifier
    controller prepends them to the action batch itself (:84-86).
(d) ``compare_to_expert`` is accepted and ignored; ``verbose_frac_display`` is accepted, the plan page shows ten plans;
    ``classifier_batch_size`` is accepted, the device scores a chunk's frames in one call.
"""
import json

import numpy as np

from ..cem_base_controller import CEMBaseController
from ..pixel_cost_controller import _default_predictor_class, build_predictor, context_states
from visual_foresight_amd.video_prediction import frame_scorer_arch


class LearnedCostController(CEMBaseController):
    """What ``ClassifierController`` and ``NCECostController`` share: predictor + scorer construction, the device path
    and the host fallback, ``_weight_scores``, the plan page."""
    HEAD = 'classifier'
    PREFIX = 'classifier'       # hyper-parameter prefix: <prefix>_conf_path, _restore_path, _batch_size

    def __init__(self, ag_params, policyparams, gpu_id, ngpu):
        """
        :param ag_params: agent parameter dict (needs adim, sdim, image_height, image_width)
        :param policyparams: policy parameter dict (overrides of the HParams defaults)
        :param gpu_id: first GPU to use
        :param ngpu: number of GPUs to use
        """
        CEMBaseController.__init__(self, ag_params, policyparams)
        predictor_class = self._hp.predictor_class
        if predictor_class is None:
            predictor_class = _default_predictor_class(ag_params.get('ncam', 1))
        horizon = self._hp.nactions * self._hp.get('repeat', 1)
        self.predictor = build_predictor(self, predictor_class, ag_params, gpu_id, ngpu, 1, horizon)
        self._net_context = self.predictor.n_context
        self._n_pred = self.predictor.sequence_length - self._net_context
        self._img_height, self._img_width = [ag_params['image_height'], ag_params['image_width']]
        self._n_cam = getattr(self.predictor, 'n_cam', 1)
        self.scorer = self._build_scorer()

        self._images = None
        self._expert_images = None
        self._expert_score = None
        self._goal_image = None
        self._start_image = None
        self._verbose_worker = None
        self.cost_perstep = None        # [M, T] raw cost (summed over views) of the last scoring call

    def _scorer_hparams(self):
        hp = {}
        conf = self._hp.get(self.PREFIX + '_conf_path')
        if conf:
            with open(conf) as f:
                hp.update(json.load(f))
        hp.update(image_height=self._img_height, image_width=self._img_width, ncam=self._n_cam, head=self.HEAD)
        return hp

    def _build_scorer(self):
        from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer, HostFrameScorer
        hp = self._scorer_hparams()
        path = self._hp.get(self.PREFIX + '_restore_path')
        if hasattr(self.predictor, 'score_frames'):
            hp['max_frames'] = self.predictor.run_batch_size * self._n_pred
            return HipFrameScorer(path, hp, self.predictor.device).restore()
        return HostFrameScorer(path, hp).restore()

    def reset(self):
        self._expert_score = None
        self._images = None
        self._expert_images = None
        self._goal_image = None
        self._start_image = None
        self._verbose_worker = None
        return super(LearnedCostController, self).reset()

    # ------------------------------------------------------------------ rollout scoring
    def _goal_enc(self):
        return None

    def _with_centre_distribution(self, context):
        """``context`` plus the one distribution channel the network carries, switched on at the image centre - or, for a
        frames-only predictor (``predictor.frames_only``: no such channel, ``FramesOnlyHipVPredEvaluation``), as it is."""
        if getattr(self.predictor, 'frames_only', False):
            return context
        one_hot = np.zeros((self._net_context, self._n_cam, self._img_height, self._img_width, 1), np.float32)
        one_hot[:, :, self._img_height // 2, self._img_width // 2, :] = 1.
        return dict(context, context_pixel_distributions=one_hot)

    def evaluate_rollouts(self, actions, cem_itr):
        context = {
            "context_frames": self._images,
            "context_actions": self._sampler.chosen_actions,
            "context_states": context_states(self),
        }
        goal_enc = self._goal_enc()
        if hasattr(self.predictor, 'score_frames'):
            scores = self.predictor.score_frames(context, {'actions': actions}, self.scorer, goal_enc=goal_enc,
                                                 finalweight=self._hp.finalweight)
            self.cost_perstep = self.predictor.last_frame_cost_per_step
        else:
            prediction = self.predictor(self._with_centre_distribution(context), {'actions': actions})
            scores = self._host_scores(prediction['predicted_frames'], goal_enc)
        self._log_and_page(cem_itr, scores, context, actions)
        return scores

    def _log_and_page(self, cem_itr, scores, context, actions):
        """When the iteration is the one to show: its best scores and plan page."""
        if self._verbose_condition(cem_itr):
            self._logger.log('best scores itr {}: {}'.format(cem_itr, np.sort(scores)[:10]))
            if self._verbose_worker is not None:
                self._put_plan_page(cem_itr, scores, context, actions)

    # ------------------------------------------------------------------ device-resident CEM
    def _device_cem_plan(self):
        return self._device_cem_shape('score_frames_device', LearnedCostController.evaluate_rollouts, pages_only=True)

    def _score_device_candidates(self, candidates, itr):
        context = {
            "context_frames": self._images,
            "context_actions": self._sampler.chosen_actions,
            "context_states": context_states(self),
        }
        scores_dev = self.predictor.score_frames_device(context, candidates, self.scorer, goal_enc=self._goal_enc(),
                                                        finalweight=self._hp.finalweight)
        return scores_dev, context

    def _device_cem_downloads(self):
        return [self.predictor.last_frame_rows_dev]

    def _device_cem_finish(self, last, scores, context, downloaded):
        self.cost_perstep = np.ascontiguousarray(downloaded[0][:, 1:])
        self._log_earlier_iterations(last)
        self._log_and_page(last, scores, context, None)

    def _host_scores(self, gen_images, goal_enc):
        """Host scoring of materialised frames ``[M, T, ncam, H, W, 3]`` (in [0, 1])."""
        gen_images = np.asarray(gen_images)
        M, T = gen_images.shape[:2]
        head_out = self.scorer.embed(gen_images.reshape((M * T,) + gen_images.shape[2:]))
        raw = self._raw_scores(head_out.reshape(M, T, self._n_cam, -1), goal_enc)
        self.cost_perstep = raw
        return self._weight_scores(raw)

    def _raw_scores(self, head_out, goal_enc):
        """Head outputs ``[M, T, ncam, 2]`` -> raw cost ``[M, T]`` (:96-104)."""
        return frame_scorer_arch.classifier_raw_cost(head_out)

    def _weight_scores(self, raw_scores):
        return frame_scorer_arch.weight_scores(raw_scores, self._hp.finalweight)

    def _page_goal_images(self):
        return None

    def _put_plan_page(self, cem_itr, scores, context, actions):
        """The reference's page (:107-131): start image, the predicted frames of the ten best plans, their scores -
        rendered by the predictor's ``render_plans`` where the last rollout lies, else on the host."""
        from ..visualizer import plan_page
        self.visualize_indices = scores.argsort()[:plan_page.N_PLANS]
        rendered = plan_page.render_for_page(self.predictor, self.visualize_indices,
                                             self._with_centre_distribution(context), actions, want_distributions=False)
        for message in plan_page.build_plan_messages(
                self._t, cem_itr, self._images[-1], scores[self.visualize_indices], rendered['frames'],
                goal_images=self._page_goal_images(), img_height=self._hp.verbose_img_height,
                extensions=plan_page.asset_extensions(self._verbose_worker)):
            self._verbose_worker.put(message)


class ClassifierController(LearnedCostController):
    HEAD = 'classifier'
    PREFIX = 'classifier'

    def _default_hparams(self):
        defaults = [
            ('predictor_class', None),      # None -> HipVPredEvaluation
            ('model_path', ''),
            ('vpred_batch_size', 200),
            ('finalweight', 100),
            ('classifier_conf_path', ''),
            ('classifier_restore_path', ''),
            ('classifier_batch_size', 200),
            ('state_append', None),
            ('compare_to_expert', False),
            ('verbose_img_height', 128),
            ('verbose_frac_display', 0.),
        ]
        params = super(ClassifierController, self)._default_hparams()
        for name, value in defaults:
            params.add_hparam(name, value)
        return params

    def act(self, t=None, i_tr=None, images=None, state=None, verbose_worker=None):
        """
        :param images: uint8 history ``[t+1, ncam, H, W, 3]``
        :param state: state history ``[t+1, sdim]``
        """
        self._images = images
        self._verbose_worker = verbose_worker
        return super(ClassifierController, self).act(t, i_tr, state)
