"""Several pixel-cost planning problems on ONE predictor: their CEM iterations run in lock step and every iteration's
candidates of all problems are scored by one batched rollout (``HipVPredEvaluation.score_batch``: one ``vf_set_contexts``,
one ``vf_rollout``, one ``vf_group_pixel_scores``).

The reference runs independent planning problems side by side as separate workers with a policy each (``sim/run.py
--nworkers``); a small problem - a controller's ``num_samples`` rollouts - does not fill an MI355X, G of them in one
launch come closer.  ``BatchedPixelCostPlanner`` owns G ``PixelCostController`` instances that share one predictor and
plays their ``act`` calls together.  There is one source of the CEM loop (``CEMBaseController._cem_iterations``): every
controller proposes from its own sampler, selects its own elites and refits; only the scoring step is supplied from here.
No threads.

Samplers that draw from the global ``np.random`` stream (``GaussianCEMSampler`` and the other reference samplers)
interleave their draws across the problems: they plan correctly, but a problem's run is not the run a single controller
would have made with the same global seed.  The Philox samplers with a ``sampler_seed`` of their own are - bit for bit on a
predictor whose batched scores are its single scores (``tests/test_batched_planner.py``), to the rounding of the grouped
cost on the device (``tests/test_gpu_batched_contexts.py``).  With Philox samplers the planner uses their host form; the
device-resident CEM loop per problem is a follow-up: an explicit ``device_cem=True`` is refused, and a
Philox sampler's DEFAULT ``device_cem`` (True) is set to False for the planner's controllers without a word.
``policyparams`` is one dictionary for all problems or a list of G; what shapes the one rollout and the one predictor
(``num_samples``, the horizon, ``iterations``, ``finalweight``, ``predictor_class``, ``model_path``, ...) must agree.
"""
import numpy as np

from .pixel_cost_controller import PixelCostController, _default_predictor_class


class BatchedPixelCostPlanner(object):
    def __init__(self, ag_params, policyparams, gpu_id, ngpu, n_problems):
        """
        :param ag_params, policyparams, gpu_id, ngpu: what every ``PixelCostController`` of the planner is built with
        :param n_problems: G, the number of planning problems (controllers) that share the predictor
        """
        n_problems = int(n_problems)
        if n_problems < 1:
            raise ValueError('BatchedPixelCostPlanner needs at least one problem, got %d' % n_problems)
        # one dictionary for every problem, or a list of G of them (a sampler_seed each, say)
        per_problem = [dict(p) for p in policyparams] if isinstance(policyparams, (list, tuple)) else \
            [dict(policyparams) for _ in range(n_problems)]
        if len(per_problem) != n_problems:
            raise ValueError('BatchedPixelCostPlanner: %d policyparams for %d problems' % (len(per_problem), n_problems))
        shared = []     # the one predictor
        for params in per_problem:
            self._check_policyparams(params)
            for name in ('predictor_class', 'model_path'):     # ... which one model serves: the problems may not name two
                if params.get(name) != per_problem[0].get(name):
                    raise ValueError('BatchedPixelCostPlanner: the problems share one predictor and differ in %r (%r, %r)'
                                     % (name, per_problem[0].get(name), params.get(name)))
        for params in per_problem:
            params['predictor_class'] =self._predictor_factory(
                shared, params.get('predictor_class') or _default_predictor_class(ag_params.get('ncam', 1)), n_problems)

        self.n_problems = n_problems
        self.controllers = [PixelCostController(ag_params, params, gpu_id, ngpu) for params in per_problem]
        self.predictor = shared[0]
        hp = self.controllers[0]._hp
        for ctrl in self.controllers[1:]:       # one rollout serves all: its shape and its cost are everybody's
            for name in ('num_samples', 'iterations', 'finalweight', 'only_take_first_view', 'designated_pixel_count',
                         'append_action'):
                if ctrl._hp.get(name) != hp.get(name):
                    raise ValueError('BatchedPixelCostPlanner: the problems differ in %r (%r, %r)'
                                     % (name, hp.get(name), ctrl._hp.get(name)))
            if ctrl._plan_horizon() != self.controllers[0]._plan_horizon():
                raise ValueError('BatchedPixelCostPlanner: the problems differ in their planning horizon')
        if hp.num_samples > hp.vpred_batch_size:
            raise ValueError('BatchedPixelCostPlanner keeps all rows of a call resident in one chunk: num_samples (%d) may '
                             'not exceed vpred_batch_size (%d)' % (hp.num_samples, hp.vpred_batch_size))
        if not hasattr(self.predictor, 'score_batch'):
            raise ValueError('BatchedPixelCostPlanner needs a predictor with score_batch; %s has none'
                             % type(self.predictor).__name__)
        refusal = getattr(self.predictor, 'score_batch_refusal', lambda: None)()
        if refusal:
            raise ValueError('BatchedPixelCostPlanner: ' + refusal)

    @staticmethod
    def _check_policyparams(policyparams):
        """The refusals a problem's policy hyper-parameters can earn; the device-resident CEM route is switched off."""
        controller_class = policyparams.get('type', PixelCostController)
        if controller_class is not PixelCostController:
            raise ValueError('BatchedPixelCostPlanner plans with PixelCostController itself; %s (trade-off weights, '
                             'registration) is not batched' % getattr(controller_class, '__name__', controller_class))
        if policyparams.get('verbose', True):
            raise ValueError("BatchedPixelCostPlanner renders no plan pages: set the policy hyper-parameter 'verbose' to False")
        if policyparams.get('device_cem', False):
            raise ValueError("BatchedPixelCostPlanner runs the samplers' host form: the device-resident CEM route "
                             "(policy hyper-parameter 'device_cem') is not batched; set it to False")
        sampler_class = policyparams.get('sampler')
        if sampler_class is not None and sampler_class.get_default_hparams().get('device_cem'):
            policyparams['device_cem'] = False      # (a Philox sampler: its host form)

    @staticmethod
    def _predictor_factory(shared, wanted_class, n_problems):
        """What a controller calls as its ``predictor_class``: the first call builds the predictor, for the rows of ALL
        problems, the others get that instance."""
        def predictor_factory(model_path, hparams, n_gpus=1, first_gpu=0):
            if not shared:
                hp = dict(hparams, run_batch_size=n_problems * int(hparams['run_batch_size']))
                shared.append(wanted_class(model_path, hp, n_gpus=n_gpus, first_gpu=first_gpu))
            return shared[0]
        for name in ('wants_agent_params', 'n_context_default'):
            if hasattr(wanted_class, name):
                setattr(predictor_factory, name, getattr(wanted_class, name))
        return predictor_factory

    def reset(self):
        for ctrl in self.controllers:
            ctrl.reset()

    def act(self, requests):
        """``requests``: a list of G keyword dictionaries of ``PixelCostController.act`` -> the list of G results,
        ``{'actions', 'plan_stat'}`` each.  A controller that does not plan at this step (``t < start_planning``, inside a
        ``replan_interval``) takes no rows of the call; if none plans, nothing is launched."""
        if len(requests) != self.n_problems:
            raise ValueError('BatchedPixelCostPlanner.act wants %d requests, got %d' % (self.n_problems, len(requests)))
        planning = []
        for g, (ctrl, req) in enumerate(zip(self.controllers, requests)):
            req = dict(req)
            if req.pop('verbose_worker', None) is not None:
                raise ValueError('BatchedPixelCostPlanner renders no plan pages: verbose_worker must be None')
            t, i_tr, state = req.pop('t', None), req.pop('i_tr', None), req.pop('state', None)
            ctrl._set_task(**req)
            ctrl._state, ctrl.i_tr, ctrl._t = state, i_tr, t
            if t >= ctrl._hp.start_planning and ctrl._replan_due():
                planning.append(g)
        self._plan(planning)
        results = []
        for g, ctrl in enumerate(self.controllers):
            if ctrl._t < ctrl._hp.start_planning:
                action = ctrl._action_before_planning(ctrl._t, ctrl._state)
            else:
                # (inside a replan interval _action_from_plan advances along the standing plan)
                action = ctrl._action_from_plan(ctrl._state, planned=g in planning)
            results.append(ctrl._finish_act(ctrl._t, action))
        return results

    def _plan(self, planning):
        """One CEM call of the controllers ``planning``, in lock step: every iteration's candidates are one batched rollout."""
        if not planning:
            return
        ctrls = [self.controllers[g] for g in planning]
        hp = ctrls[0]._hp
        loops = [c._cem_iterations(c._state) for c in ctrls]
        proposals = [next(loop) for loop in loops]
        while proposals is not None:
            itr = proposals[0][1]
            assert all(p[1] == itr for p in proposals)
            actions = np.stack([p[0] for p in proposals])
            contexts = [c._rollout_context(itr) for c in ctrls]
            goals = np.stack([c._goal_pix for c in ctrls])
            scores, per_task = self.predictor.score_batch(contexts, {'actions': actions}, goals, finalweight=hp.finalweight,
                                                          only_take_first_view=hp.only_take_first_view)
            M = actions.shape[1]
            nxt = []
            for j, (c, loop) in enumerate(zip(ctrls, loops)):
                s = np.ascontiguousarray(scores[j])
                c._fused_scores_done(itr, s, per_task[j], row_base=j * M)
                try:
                    nxt.append(loop.send(s))
                except StopIteration:       # behind the last iteration (every loop has the same number of them)
                    pass
            assert len(nxt) in (0, len(loops))
            proposals = nxt or None
