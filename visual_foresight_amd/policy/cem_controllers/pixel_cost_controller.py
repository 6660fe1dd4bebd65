"""CEM controller scoring rollouts by the expected distance of designated pixels to goals.

API-compatible restatement of the reference's
``visual_mpc/policy/cem_controllers/pixel_cost_controller.py`` (ctor :20-50, defaults :52-69,
``evaluate_rollouts`` :76-133, ``_eval_pixel_cost`` :135-166, ``_expected_distance`` :168-187,
``_get_distancegrid`` :189-197, ``_switch_on_pix`` :206-215, ``act`` :217-233).

The one device crossing of the planner is ``self.predictor(context, {'actions': actions})``
(reference :83).  The default ``predictor_class`` here is the MI355X-native
``HipVPredEvaluation``; when the predictor offers the fused ``score`` entry point the
predicted videos never leave the GPU - the designated-pixel distributions are reduced to
per-sample costs on the device and only ``scores[M]`` comes back (sharded over ranks and
all-gathered when ``torch.distributed`` is initialised).  Any other predictor with the
``VPredEvaluation`` duck-type (``__call__`` returning ``predicted_frames`` /
``predicted_pixel_distributions``) is scored on the host exactly as the reference does.
"""
import numpy as np

from .cem_base_controller import CEMBaseController


def _default_predictor_class(ncam=1):
    """``HipVPredEvaluation`` rolls any number of views (``ncam`` reaches it through the predictor hparams)."""
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    return HipVPredEvaluation


def context_states(ctrl):
    """The state history a controller hands to its predictor: ``ctrl._state [t+1, sdim]`` as it is, or - with the
    ``state_append`` hyper-parameter, a list of k constants - ``[t+1, sdim + k]`` with the constants appended to every
    row, as ``pred_util.get_context`` appends them at the legacy boundary (reference ``pred_util.py:9-11``).  Experiments
    use it for state dimensions the network was trained with and the robot does not report.  The sampler keeps
    receiving the agent's own state."""
    extra = ctrl._hp.get('state_append')
    if not extra:
        return ctrl._state
    state = np.asarray(ctrl._state)
    tail = np.broadcast_to(np.asarray(extra), state.shape[:-1] + (len(extra),))
    return np.concatenate((state, tail), axis=-1)


def model_image_size(ag_params):
    """``(height, width)`` the network runs at.  The agent's ``image_height`` / ``image_width`` unless the two free-form keys
    ``model_image_height`` / ``model_image_width`` of ``ag_params`` name a smaller size of the same aspect ratio: the images
    then arrive at the camera's resolution and are shrunk to the model's (``video_prediction/resample.py``; the reference's
    agent does that itself, ``utils/im_utils.py:6-15``, and its registration controller works at both sizes).  This is the
    reference's meaning of the controllers' ``_img_height`` / ``_img_width``."""
    camera = (ag_params['image_height'], ag_params['image_width'])
    keys = ('model_image_height' in ag_params, 'model_image_width' in ag_params)
    if not any(keys):
        return camera
    if not all(keys):
        raise ValueError("ag_params: 'model_image_height' and 'model_image_width' come as a pair")
    model = (int(ag_params['model_image_height']), int(ag_params['model_image_width']))
    from visual_foresight_amd.video_prediction.resample import check_aspect
    check_aspect(camera, model)
    return model


def context_frames(ctrl):
    """The image history as the predictor takes it.  A predictor that was told the camera's size (``camera_size``:
    ``HipVPredEvaluation`` with ``camera_height`` / ``camera_width``) shrinks the frames on its device; for any other the
    last ``n_context`` frames are shrunk here, on the host (reference ``register_gtruth_controller.py:50-51``)."""
    images = ctrl._images
    if ctrl._camera_size is None or getattr(ctrl.predictor, 'camera_size', None) is not None:
        return images           # (no model-size keys: the default path hands the history on untouched)
    model = (ctrl._img_height, ctrl._img_width)
    if tuple(np.shape(images)[-3:-1]) == model:
        return images
    from visual_foresight_amd.video_prediction.resample import area_resize_host
    return area_resize_host(np.asarray(images)[-ctrl._net_context:], model)


def page_start_images(ctrl):
    """The newest observed frame as the plan page shows it: at the model's size, like the predicted frames beside it and
    the designated / goal pixels marked on it."""
    if ctrl._camera_size is None:
        return ctrl._images[-1]
    newest = np.asarray(ctrl._images[-1])
    model = (ctrl._img_height, ctrl._img_width)
    if tuple(newest.shape[-3:-1]) == model:
        return ctrl._images[-1]
    from visual_foresight_amd.video_prediction.resample import area_resize_host
    return area_resize_host(newest, model)


def build_predictor(ctrl, predictor_class, ag_params, gpu_id, ngpu, designated_pixel_count, horizon):
    """Construct and restore the video predictor of a CEM controller (reference ``pixel_cost_controller.py:29-36``) and
    raise the controller's ``start_planning`` to the network's context.  Shared by the controllers that plan on
    predicted videos (``PixelCostController`` and its variants, ``GoalImController``).  The predictor's ``sdim`` is the
    agent's plus the number of ``state_append`` constants: the width of ``context_states(ctrl)``."""
    hp = ctrl._hp
    predictor_hparams = {
        'designated_pixel_count': designated_pixel_count,
        'run_batch_size': min(hp.vpred_batch_size, hp.num_samples),
    }
    if getattr(predictor_class, 'wants_agent_params', False):
        # the HIP predictor is shape-specialised at construction (no checkpoint json to read
        # adim/sdim/size/T from), so it is told what the controller will ask of it
        predictor_hparams.update(
            adim=ctrl._adim, sdim=ctrl._sdim + len(hp.get('state_append') or ()),
            image_height=ag_params['image_height'], image_width=ag_params['image_width'],
            ncam=ag_params.get('ncam', 1),
            sequence_length=horizon + predictor_class.n_context_default)
        model = model_image_size(ag_params)
        if model != (ag_params['image_height'], ag_params['image_width']):
            # the predictor runs at the model's size and shrinks the camera-size context itself
            predictor_hparams.update(image_height=model[0], image_width=model[1],
                                     camera_height=ag_params['image_height'], camera_width=ag_params['image_width'])
    predictor = predictor_class(hp.model_path, predictor_hparams, n_gpus=ngpu, first_gpu=gpu_id)
    predictor.restore()
    if hp.start_planning < predictor.n_context - 1:
        hp.start_planning = predictor.n_context - 1
    return predictor


class PixelCostController(CEMBaseController):
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
            predictor_class = self._default_predictor_class(ag_params)
        self.predictor = build_predictor(self, predictor_class, ag_params, gpu_id, ngpu,
                                         self._hp.designated_pixel_count, self._plan_horizon())
        self._net_context = self.predictor.n_context

        self._n_desig = self._hp.designated_pixel_count
        self._img_height, self._img_width = model_image_size(ag_params)
        # the agent's image size when the model's differs from it (the two ag_params keys), else None
        self._camera_size = (ag_params['image_height'], ag_params['image_width'])
        if self._camera_size == (self._img_height, self._img_width):
            self._camera_size = None
        # the reference hard-codes 1 here (:43); multi-view predictors announce their view count
        self._n_cam = getattr(self.predictor, 'n_cam', 1)

        self._desig_pix = None
        self._goal_pix = None
        self._images = None
        if self._hp.predictor_propagation:
            self._chosen_distrib = None     # distributions of the executed plan

    def _default_predictor_class(self, ag_params):
        """The predictor built when ``predictor_class`` is None (variants override this)."""
        return _default_predictor_class(ag_params.get('ncam', 1))

    def _plan_horizon(self):
        """Number of predicted steps the sampler will produce (nactions * repeat)."""
        hp = self._hp
        return hp.nactions * hp.get('repeat', 1)

    def _default_hparams(self):
        defaults = [
            ('predictor_class', None),      # None -> HipVPredEvaluation
            ('model_path', ''),
            ('vpred_batch_size', 200),
            ('designated_pixel_count', 1),
            ('verbose_img_height', 128),
            ('predictor_propagation', False),
            ('only_take_first_view', False),
            ('state_append', None),
            ('finalweight', 10.),
        ]
        params = super(PixelCostController, self)._default_hparams()
        for name, value in defaults:
            params.add_hparam(name, value)
        return params

    def reset(self):
        super(PixelCostController, self).reset()
        if self._hp.predictor_propagation:
            self._chosen_distrib = None

    # ------------------------------------------------------------------ rollout scoring
    def _rollout_context(self, cem_itr):
        """What the predictor is told of the present at CEM iteration ``cem_itr``."""
        return {
            "context_frames": context_frames(self),
            "context_actions": self._sampler.chosen_actions,
            "context_pixel_distributions": self._make_input_distrib(cem_itr),
            "context_states": context_states(self),
        }

    def _fused_scores_done(self, cem_itr, scores, scores_per_task, row_base=0):
        """What follows the predictor's fused scores of iteration ``cem_itr``: the task log, and the distributions of the
        best plan for ``predictor_propagation``.  ``row_base``: the predictor's index of this controller's first candidate
        (``BatchedPixelCostPlanner``: the rows of several controllers lie in one rollout)."""
        self._log_task_scores(scores, scores_per_task)
        if self._hp.predictor_propagation and cem_itr == self._hp.iterations - 1:
            bestind = scores.argsort()[0]
            self._chosen_distrib = self.predictor.fetch_pixel_distributions(row_base + bestind)

    def evaluate_rollouts(self, actions, cem_itr):
        context = self._rollout_context(cem_itr)
        if hasattr(self.predictor, 'score'):
            weights = self._task_weights()
            on_device = weights is not None and getattr(self.predictor, 'supports_task_weights', False)
            kw = {'task_weights': weights} if on_device else {}
            scores, scores_per_task = self.predictor.score(
                context, {'actions': actions}, goal_pix=self._goal_pix,
                finalweight=self._hp.finalweight,
                only_take_first_view=self._hp.only_take_first_view, **kw)
            if weights is not None and not on_device:
                scores = np.sum(scores_per_task * np.asarray(weights).reshape(1, -1), axis=1)
            self._fused_scores_done(cem_itr, scores, scores_per_task)
        else:
            prediction = self.predictor(context, {'actions': actions})
            gen_images = prediction['predicted_frames']
            gen_distrib = prediction['predicted_pixel_distributions']
            scores = self._eval_pixel_cost(cem_itr, gen_distrib, gen_images)

        if self._verbose_condition(cem_itr):
            self._visualize(cem_itr, scores, context, actions)
        return scores

    def _task_weights(self):
        """Per-(camera, designated pixel) score weights, or None for the reference's plain mean."""
        return None

    # ------------------------------------------------------------------ device-resident CEM
    def _device_cem_plan(self):
        return self._pixel_cost_device_plan(PixelCostController.evaluate_rollouts)

    def _pixel_cost_device_plan(self, own_evaluate):
        """``(K, M, tail)`` when this planning call can stay on the device, else None: the refusals of
        ``_device_cem_shape`` with the predictor's ``score_device``, and trade-off weights only where the predictor applies
        them on the device.  ``own_evaluate``: the ``evaluate_rollouts`` of the class whose device hooks answer - a subclass
        that overrides it again without them plans on the host."""
        weights = self._task_weights()
        if weights is not None and not getattr(self.predictor, 'supports_task_weights', False):
            return None
        return self._device_cem_shape('score_device', own_evaluate)

    def _score_device_candidates(self, candidates, itr):
        hp = self._hp
        weights = self._task_weights()
        kw = {'task_weights': weights} if weights is not None else {}
        context = {
            "context_frames": context_frames(self),
            "context_actions": self._sampler.chosen_actions,
            "context_pixel_distributions": self._make_input_distrib(itr),
            "context_states": context_states(self),
        }
        scores_dev = self.predictor.score_device(context, candidates, goal_pix=self._goal_pix, finalweight=hp.finalweight,
                                                 only_take_first_view=hp.only_take_first_view, **kw)
        return scores_dev, context

    def _device_cem_finish(self, last, scores, context, downloaded):
        if self._hp.predictor_propagation:
            self._chosen_distrib = self.predictor.fetch_pixel_distributions(int(self._best_indices[0]))
        if self._verbose_condition(last):
            self._visualize(last, scores, context, None)

    def _visualize(self, cem_itr, scores, context=None, actions=None):
        """Plan visualisation (reference :88-131).  Without a ``verbose_worker`` (or without the rollout's inputs) the
        ten best scores are logged.  With one, the plans ``scores.argsort()[:10]`` are rendered - by the predictor's
        ``render_plans`` where the last rollout lies, or on the host from ``self.predictor(context, ...)`` of those
        plans - and the page's messages (``visualizer/plan_page.py``) are ``put`` on the worker."""
        self._logger.log('best scores itr {}: {}'.format(cem_itr, np.sort(scores)[:10]))
        worker = getattr(self, '_verbose_worker', None)
        if worker is None or context is None:
            return
        from .visualizer import plan_page
        self.visualize_indices = scores.argsort()[:plan_page.N_PLANS]
        rendered = plan_page.render_for_page(self.predictor, self.visualize_indices, context, actions)
        for message in plan_page.build_plan_messages(
                self._t, cem_itr, page_start_images(self), scores[self.visualize_indices], rendered['frames'],
                rendered['distributions'], desig_pix=self._desig_pix, goal_pix=self._goal_pix,
                img_height=self._hp.verbose_img_height, extensions=plan_page.asset_extensions(worker)):
            worker.put(message)

    def _log_task_scores(self, scores, scores_per_task):
        bestind = scores.argsort()[0]
        for icam in range(self._n_cam):
            for p in range(self._n_desig):
                col = p + icam * self._n_desig
                if col < scores_per_task.shape[1]:
                    self._logger.log('best flow score of task {} cam{}  :{}'.format(
                        p, icam, np.min(scores_per_task[:, col])))
                    self._logger.log('flow score of best traj for task{} cam{} :{}'.format(
                        p, icam, scores_per_task[bestind, col]))

    def _eval_pixel_cost(self, cem_itr, gen_distrib, gen_images):
        """Host scoring of materialised distributions ``[M, T, ncam, H, W, ndesig]``."""
        per_task = []
        for icam in range(self._n_cam):
            for p in range(self._n_desig):
                grid = self._get_distancegrid(self._goal_pix[icam, p])
                per_task.append(self._expected_distance(icam, p, gen_distrib[:, :, icam, :, :, p], grid,
                                                        normalize=True))
        scores_per_task = np.stack(per_task, axis=1)
        if self._hp.only_take_first_view:
            scores_per_task = scores_per_task[:, 0][:, None]
        weights = self._task_weights()
        if weights is not None:
            scores = np.sum(scores_per_task * np.asarray(weights).reshape(1, -1), axis=1)
        else:
            scores = np.mean(scores_per_task, axis=1)
        self._log_task_scores(scores, scores_per_task)

        if self._hp.predictor_propagation and cem_itr == self._hp.iterations - 1:
            # propagate the distributions of the plan that will actually be executed
            self._chosen_distrib = gen_distrib[scores.argsort()[0]]
        return scores

    def _expected_distance(self, icam, idesig, gen_distrib, distance_grid, normalize=True):
        """score_b = sum_t w_t * E_{p_bt}[distance] / sum_t w_t, w = (1, ..., 1, finalweight).

        :param gen_distrib: ``[batch, t, r, c]``
        :param distance_grid: ``[r, c]``
        """
        assert len(gen_distrib.shape) == 4
        t_mult = np.ones([self.predictor.sequence_length - self._net_context])
        t_mult[-1] = self._hp.finalweight

        p = gen_distrib.copy()
        if normalize:
            p /= np.sum(np.sum(p, axis=2), 2)[:, :, None, None]
        p *= distance_grid[None, None]
        per_step = np.sum(np.sum(p, axis=2), 2)
        per_step *= t_mult[None]
        return np.sum(per_step, axis=1) / np.sum(t_mult)

    def _get_distancegrid(self, goal_pix):
        """D[i, j] = || goal_pix - (i, j) ||_2 in (row, col) order, float64."""
        rows = np.arange(self._img_height, dtype=np.float64)[:, None] - np.float64(goal_pix[0])
        cols = np.arange(self._img_width, dtype=np.float64)[None, :] - np.float64(goal_pix[1])
        self._logger.log('making distance grid with goal_pix', goal_pix)
        return np.sqrt(rows * rows + cols * cols)

    # ------------------------------------------------------------------ designated pixels
    def _make_input_distrib(self, itr):
        if self._hp.predictor_propagation and self._chosen_distrib is not None:
            # let the predictor's own flow carry the distribution forward, no correction
            return self._chosen_distrib[-self._net_context:]
        return self._switch_on_pix(self._desig_pix)

    def _switch_on_pix(self, desig):
        one_hot = np.zeros((self._net_context, self._n_cam, self._img_height, self._img_width,
                            self._n_desig), dtype=np.float32)
        hi = np.array([self._img_height, self._img_width]).reshape((1, 2)) - 1
        desig = np.clip(desig, np.zeros((1, 2)), hi).astype(int)
        for icam in range(self._n_cam):
            for p in range(self._n_desig):
                one_hot[:, icam, desig[icam, p, 0], desig[icam, p, 1], p] = 1.
                self._logger.log('using desig pix', desig[icam, p, 0], desig[icam, p, 1])
        return one_hot

    def act(self, t=None, i_tr=None, desig_pix=None, goal_pix=None, images=None, state=None,
            verbose_worker=None):
        """
        :param t: the controller's time step
        :param desig_pix: designated pixels, (row, col) in small-image coordinates
        :param goal_pix: goal pixels, same coordinates; both reshapeable to [ncam, ndesig, 2]
        :param images: uint8 history ``[t+1, ncam, H, W, 3]``
        :param state: state history ``[t+1, sdim]``
        """
        self._set_task(desig_pix, goal_pix, images, verbose_worker)
        return super(PixelCostController, self).act(t, i_tr, state)

    def _set_task(self, desig_pix, goal_pix, images, verbose_worker=None):
        """The task part of an ``act`` call: where the designated pixels are and should go, and the image history."""
        self._desig_pix = np.array(desig_pix).reshape((self._n_cam, self._n_desig, 2))
        self._goal_pix = np.array(goal_pix).reshape((self._n_cam, self._n_desig, 2))
        self._images = images
        self._verbose_worker = verbose_worker
