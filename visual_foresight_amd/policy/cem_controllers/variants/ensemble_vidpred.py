"""CEM planning with an ensemble of independently trained predictors: per step, cost = member mean + lambda * variance.

Restates the reference's ``visual_mpc/policy/cem_controllers/variants/ensemble_vidpred.py`` (defaults :12-16, cost
:32-61) at the same import path.  Hyper-parameters are the parent's plus ``num_ensembles`` (4) and
``lambda_variance`` (0.1).  The default predictor is ``EnsembleHipPredictor``: its fused ``score`` reduces the members'
resident cost sums on the device and hands back ``cost_perstep`` as well.  Any predictor without ``score`` is scored on
the host from the ``ensemble_pixel_distributions`` [E, M, T, ncam, H, W, nd] its ``__call__`` returns, exactly as the
reference's ``_expected_distance`` does.

Departure: the reference interleaves the members in blocks of its tower batch (``_net_bsize``) and so needs
``M % (batch / E) == 0``; both are artefacts of its tower batching and are not carried over - members are a leading
axis here and any M works.
"""
import numpy as np

from ..pixel_cost_controller import PixelCostController, context_states


def ensemble_expected_distance(gen_distrib, distance_grid, lambda_variance, finalweight, normalize=True):
    """Reference ``_expected_distance`` of the ensemble variant on member-major distributions, in the reference's
    arithmetic (the in-place steps keep the distributions' dtype: float32 in, float32 per-step costs).

    :param gen_distrib: ``[E, M, T, r, c]``
    :param distance_grid: ``[r, c]``
    :return: (scores [M], per-step cost [M, T] = mean_E + lambda * var_E of the expected distance)
    """
    assert gen_distrib.ndim == 5
    T = gen_distrib.shape[2]
    t_mult = np.ones([T])
    t_mult[-1] = finalweight
    p = gen_distrib.copy()
    if normalize:
        p /= np.sum(np.sum(p, axis=3), 3)[:, :, :, None, None]
    p *= distance_grid[None, None, None]
    per_member = np.sum(np.sum(p, axis=3), 3)                                   # [E, M, T]
    per_step = np.mean(per_member, axis=0) + lambda_variance * np.var(per_member, axis=0)
    scores = per_step.copy()
    scores *= t_mult[None]          # in place, in the distributions' precision, as the reference does
    return np.sum(scores, axis=1) / np.sum(t_mult), per_step


class CEM_Controller_Ensemble_Vidpred(PixelCostController):
    def __init__(self, ag_params, policyparams, gpu_id, ngpu):
        super(CEM_Controller_Ensemble_Vidpred, self).__init__(ag_params, policyparams, gpu_id, ngpu)
        self.cost_perstep = None        # [M, ncam, nd, T] of the last scoring call

    def _default_hparams(self):
        params = super(CEM_Controller_Ensemble_Vidpred, self)._default_hparams()
        params.add_hparam('num_ensembles', 4)
        params.add_hparam('lambda_variance', 0.1)
        return params

    def _default_predictor_class(self, ag_params):
        from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor
        return EnsembleHipPredictor.with_options(num_ensembles=self._hp.num_ensembles,
                                                 lambda_variance=self._hp.lambda_variance)

    def evaluate_rollouts(self, actions, cem_itr):
        if hasattr(self.predictor, 'score'):
            scores = super(CEM_Controller_Ensemble_Vidpred, self).evaluate_rollouts(actions, cem_itr)
            cps = self.predictor.last_cost_per_step                                 # [M, ncam*nd, T]
            self.cost_perstep = cps.reshape(cps.shape[0], self._n_cam, self._n_desig, cps.shape[2])
            return scores
        context = {
            "context_frames": self._images,
            "context_actions": self._sampler.chosen_actions,
            "context_pixel_distributions": self._make_input_distrib(cem_itr),
            "context_states": context_states(self),
        }
        prediction = self.predictor(context, {'actions': actions})
        scores = self._eval_pixel_cost(cem_itr, prediction['ensemble_pixel_distributions'],
                                       prediction['predicted_frames'])
        if self._verbose_condition(cem_itr):
            self._visualize(cem_itr, scores)
        return scores

    # ------------------------------------------------------------------ device-resident CEM
    def _device_cem_plan(self):
        """The parent's refusals against this class's own ``evaluate_rollouts``, with a predictor that keeps the ensemble's
        cost rows on the device (``EnsembleHipPredictor.score_device``)."""
        if not hasattr(self.predictor, 'last_cost_rows_dev'):
            return None
        return self._pixel_cost_device_plan(CEM_Controller_Ensemble_Vidpred.evaluate_rollouts)

    def _device_cem_downloads(self):
        """The last iteration's rows ``[M, score | per task | per task x step]``: the per-step columns are ``cost_perstep``."""
        return [self.predictor.last_cost_rows_dev]

    def _device_cem_finish(self, last, scores, context, downloaded):
        _, per_task, cps = self.predictor.split_cost_rows(downloaded[0])
        if self._hp.only_take_first_view:
            per_task = per_task[:, :1]
        self.predictor.last_cost_per_step = cps
        self.cost_perstep = cps.reshape(cps.shape[0], self._n_cam, self._n_desig, cps.shape[2])
        self._log_task_scores(scores, per_task)
        super(CEM_Controller_Ensemble_Vidpred, self)._device_cem_finish(last, scores, context, downloaded)

    def _visualize(self, cem_itr, scores, context=None, actions=None):
        """The reference's ensemble controller has no plan page: the best scores are logged."""
        self._logger.log('best scores itr {}: {}'.format(cem_itr, np.sort(scores)[:10]))

    def _eval_pixel_cost(self, cem_itr, gen_distrib, gen_images):
        """Host scoring of member-major distributions ``[E, M, T, ncam, H, W, ndesig]``."""
        E, M, T = gen_distrib.shape[:3]
        self.cost_perstep = np.zeros((M, self._n_cam, self._n_desig, T))
        per_task = []
        for icam in range(self._n_cam):
            for p in range(self._n_desig):
                grid = self._get_distancegrid(self._goal_pix[icam, p])
                per_task.append(self._expected_distance(icam, p, gen_distrib[:, :, :, icam, :, :, p], grid))
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
            self._chosen_distrib = np.mean(gen_distrib[:, scores.argsort()[0]], axis=0)
        return scores

    def _expected_distance(self, icam, idesig, gen_distrib, distance_grid, normalize=True):
        """:param gen_distrib: ``[E, M, T, r, c]``; sets ``cost_perstep[:, icam, idesig]``."""
        scores, per_step = ensemble_expected_distance(gen_distrib, distance_grid, self._hp.lambda_variance,
                                                      self._hp.finalweight, normalize)
        self.cost_perstep[:, icam, idesig] = per_step
        return scores
