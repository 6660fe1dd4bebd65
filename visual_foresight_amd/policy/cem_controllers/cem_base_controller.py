"""Cross-entropy-method planner: propose action sequences, score them, refit on the best.

API-compatible with the reference's ``visual_mpc/policy/cem_controllers/cem_base_controller.py``
(class ``CEMBaseController`` :7; hyper-parameter defaults :42-64; sampler-default merge :66-76;
``perform_CEM`` :85-116; ``act`` :127-169) - same constructor, hyper-parameter names and defaults,
``plan_stat`` keys and replan schedule, so reference experiment files drive it unchanged (pinned
by tests/test_host_golden.py against traces of the reference itself).

Subclasses implement ``evaluate_rollouts(actions, cem_itr) -> scores[M]`` (lower is better).  All
math here is small float64 host work.  The elites are ``argsort(scores)[:K]`` on the host; in the
multi-GPU build the predictor has already all-gathered the scores, so every rank picks the same.
"""
import numpy as np

from visual_foresight_amd.policy.policy import Policy
from visual_foresight_amd.utils.logger import Logger
from .samplers import GaussianCEMSampler

# (name, default) in registration order
CEM_HPARAMS = (
    ('append_action', None),                        # constant tail appended to every sampled action
    ('verbose', True),
    ('verbose_every_iter', False),
    ('logging_dir', ''),
    ('hard_coded_start_action', None),
    ('context_action_weight', [0.5, 0.5, 0.05, 1]),  # scale of the random actions before planning starts
    ('zeros_for_start_frames', True),
    ('replan_interval', 0),                          # 0: plan at every step
    ('sampler', GaussianCEMSampler),
    ('T', 15),                                       # planning horizon
    ('iterations', 3),
    ('num_samples', 200),
    ('selection_frac', 0.),                          # elite fraction; 0 -> minimum_selection
    ('start_planning', 0),
    ('minimum_selection', 10),
)


class CEMBaseController(Policy):
    def __init__(self, ag_params, policyparams):
        self._hp = self._default_hparams()
        self._override_defaults(policyparams)
        self.agentparams = ag_params
        self._adim, self._sdim = ag_params['adim'], ag_params['sdim']
        assert self._hp.minimum_selection > 0, "must take at least 1 sample for refitting"

        if self._hp.logging_dir:
            log_name = 'cem{}log.txt'.format(ag_params['gpu_id'])
            self._logger = Logger(self._hp.logging_dir, log_name)
        else:
            self._logger = Logger(printout=True, mute=not self._hp.verbose)
        self._logger.log('init CEM controller')

        self._n_iter = self._hp.iterations
        self._sampler = None
        self._state = None
        self._t = None
        self._t_since_replan = None
        self._best_indices = None
        self._best_actions = None

    # ------------------------------------------------------------------ configuration
    def _default_hparams(self):
        params = super(CEMBaseController, self)._default_hparams()
        for name, default in CEM_HPARAMS:
            params.add_hparam(name, default)
        return params

    def _override_defaults(self, policyparams):
        """Sampler defaults join the hyper-parameters first, then the user's overrides apply."""
        sampler_class = policyparams.get('sampler', GaussianCEMSampler)
        for name, default in sampler_class.get_default_hparams().items():
            if name in self._hp:
                print('Warning default value for {} already set!'.format(name))
                self._hp.set_hparam(name, default)
            else:
                self._hp.add_hparam(name, default)
        super(CEMBaseController, self)._override_defaults(policyparams)
        self._hp.sampler = sampler_class       # the class object itself, not a type-coerced copy

    def reset(self):
        """Fresh sampler and empty planning statistics; called before every rollout."""
        self._sampler = self._hp.sampler(self._hp, self._adim, self._sdim)
        self._t_since_replan = None
        self._best_indices, self._best_actions = None, None
        self.plan_stat = {}

    # ------------------------------------------------------------------ planning
    def _elite_count(self):
        hp = self._hp
        if not hp.selection_frac:
            return hp.minimum_selection
        return max(int(hp.selection_frac * hp.num_samples), hp.minimum_selection)

    def _append_constant(self, actions):
        tail = np.array(self._hp.append_action)[None, None]
        tail = np.tile(tail, [self._hp.num_samples, actions.shape[1], 1])
        return np.concatenate((actions, tail), axis=-1)

    def perform_CEM(self, state):
        plan = self._device_cem_plan()
        if plan is not None:
            return self._perform_device_CEM(state, plan)
        steps = self._cem_iterations(state)
        proposal = next(steps)
        while proposal is not None:
            scores = self.evaluate_rollouts(*proposal)
            try:
                proposal = steps.send(scores)
            except StopIteration:       # behind the last iteration
                proposal = None

    def _cem_iterations(self, state):
        """The host CEM loop as a generator: yields ``(candidates, itr)`` and is sent their ``scores [M]``; it selects the
        elites, refits and proposes again, and ends behind the last iteration.  ``perform_CEM`` sends it
        ``evaluate_rollouts``' scores; ``BatchedPixelCostPlanner`` steps the loops of several controllers side by side and
        sends each the scores one batched rollout gave its candidates - the loop itself has this one source."""
        hp = self._hp
        self._logger.log('starting cem at t{}...'.format(self._t))
        n_elite = self._elite_count()
        n_tail = len(hp.append_action) if hp.append_action else 0

        candidates = self._sampler.sample_initial_actions(self._t, hp.num_samples, state[-1])
        for itr in range(self._n_iter):
            if n_tail:
                candidates = self._append_constant(candidates)
            self._logger.log('iteration: ', itr)

            scores = yield candidates, itr
            assert scores.shape == (candidates.shape[0],), "score shape should be (n_actions,)"
            self.plan_stat['scores_itr{}'.format(itr)] = scores

            select = getattr(self._sampler, 'select_elites', None)      # a sampler may define the order of the elites
            self._best_indices = select(scores, n_elite) if select else scores.argsort()[:n_elite]
            self._best_actions = candidates[self._best_indices]

            if itr + 1 < self._n_iter:      # refit on the elites (without the appended constants)
                elites = self._best_actions.copy()
                if n_tail:
                    elites = elites[:, :, :-n_tail]
                candidates = self._sampler.sample_next_actions(
                    hp.num_samples, elites, scores[self._best_indices].copy())
        self._t_since_replan = 0

    def evaluate_rollouts(self, actions, cem_itr):
        raise NotImplementedError

    # ------------------------------------------------------------------ device-resident CEM
    keep_device_candidates = False      # debug: keep every iteration's candidates of a device-route call (device_candidates)

    def _device_cem_plan(self):
        """Hook: ``(K, M, tail)`` when this planning call can stay on the device, else None (the host route).  A controller
        that scores on the device answers with ``_device_cem_shape``."""
        return None

    def _score_device_candidates(self, candidates, itr):
        """Hook: score the device candidates ``[M, T, adim + tail]`` of iteration ``itr`` -> (device float64 scores ``[M]``,
        the context the rollout saw).  Only enqueues."""
        raise NotImplementedError

    def _device_cem_downloads(self):
        """Hook: device tensors of the last iteration that join the call's one download."""
        return []

    def _device_cem_finish(self, last, scores, context, downloaded):
        """Hook, after the download: what the host route sets from the last iteration ``last`` (``scores [M]`` of it, the
        host copies ``downloaded`` of ``_device_cem_downloads``)."""

    def _device_cem_shape(self, entry, own_evaluate, pages_only=False):
        """The refusals every device route shares -> ``(K, M, tail)`` or None: the sampler names a device driver
        (``device_cem_driver``: the Philox samplers) and has ``device_cem``, the predictor offers ``entry`` and its refusal
        (``<entry>_refusal``, or the one the frame entries share) is silent, the rollouts are scored by ``own_evaluate`` (the
        controller class's own ``evaluate_rollouts``) and every iteration's page is not asked for: ``verbose_every_iter``, or,
        with ``pages_only`` (a controller whose ``_device_cem_finish`` logs every iteration, ``_log_earlier_iterations``),
        ``verbose_every_iter`` together with a verbose worker to put the pages on."""
        from .samplers.philox_gaussian_sampler import MAX_K, MAX_SAMPLES
        hp, sampler, pred = self._hp, self._sampler, self.predictor
        if getattr(sampler, 'device_cem_driver', None) is None or not hp.get('device_cem'):
            return None
        refusal = 'score_device_refusal' if entry == 'score_device' else 'frame_score_device_refusal'
        if not hasattr(pred, entry) or getattr(pred, refusal, lambda: None)():
            return None
        if type(self).evaluate_rollouts is not own_evaluate:
            return None
        if hp.verbose and hp.verbose_every_iter:    # only the last rollout is resident when the call is through
            if not pages_only or getattr(self, '_verbose_worker', None) is not None:
                return None
        tail = list(hp.append_action) if hp.append_action else []
        K = self._elite_count()
        M = sampler.device_draws(self._t, hp.num_samples)
        # (the caller's action width: a stochastic predictor's engine takes adim + zdim, the latents are folded in later)
        width = pred._adim_in() if hasattr(pred, '_adim_in') else pred.cfg.adim
        if not (2 <= K <= min(MAX_K, M) and M <= MAX_SAMPLES) or width != sampler.action_width() + len(tail):
            return None
        return K, M, tail

    def _log_earlier_iterations(self, last):
        """With ``verbose_every_iter``: the best-scores line of every iteration before ``last``, as the host route logs it."""
        if self._hp.verbose and self._hp.verbose_every_iter:
            for itr in range(last):
                self._logger.log('best scores itr {}: {}'.format(itr, np.sort(self.plan_stat['scores_itr{}'.format(itr)])[:10]))

    def _perform_device_CEM(self, state, plan):
        """One planning call on the device: sample, score, select the elites and refit are enqueued for every iteration, then
        one download."""
        from . import device_cem
        hp, sampler, pred = self._hp, self._sampler, self.predictor
        K, M, tail = plan
        torch = pred._torch
        self._logger.log('starting cem at t{} (device route)...'.format(self._t))
        driver = getattr(device_cem, sampler.device_cem_driver)
        dc = getattr(self, '_device_cem', None)
        if type(dc) is not driver or (dc.K, dc.n_iter, dc.max_samples) != (K, self._n_iter, hp.num_samples):
            dc = self._device_cem = driver(sampler, K, self._n_iter, hp.num_samples, pred.device, tail)
        with torch.cuda.device(pred.device):
            dc.begin(sampler, self._t, M, tail, state[-1])
            for itr in range(self._n_iter):
                self._logger.log('iteration: ', itr)
                candidates = dc.sample(itr, M, sampler.next_call())
                scores_dev, context = self._score_device_candidates(candidates, itr)
                dc.scores[itr, :M].copy_(scores_dev)
                dc.refit(itr, scores_dev, candidates)       # (the last one names the final elites)
            # the one download of the call: scores, elite indices, final elite plans, what the driver adds (trial counts,
            # capped flags) and what the controller adds (the last iteration's cost rows)
            extra = dc.downloads(M)
            own = self._device_cem_downloads()
            parts = [dc.scores[:, :M], dc.elite_index, dc.elite_plans] + extra + own
            if self.keep_device_candidates:
                parts.append(dc.actions[:, :M])
            packed = torch.cat([p.reshape(-1).to(torch.float64) for p in parts]).cpu().numpy()
        sizes = np.cumsum([0] + [p.numel() for p in parts])
        host = [packed[a:b].reshape(tuple(p.shape)) for p, a, b in zip(parts, sizes[:-1], sizes[1:])]
        scores, elite_index, elite_plans = host[:3]
        pred._check_scores(scores.reshape(-1))
        for itr in range(self._n_iter):
            self.plan_stat['scores_itr{}'.format(itr)] = scores[itr].copy()
        self._best_indices = elite_index[-1].astype(np.int64)
        self._best_actions = elite_plans.copy()
        dc.finish(sampler, host[3:3 + len(extra)])
        n_own = 3 + len(extra) + len(own)
        if self.keep_device_candidates:
            self.device_candidates = [c.astype(np.float32) for c in host[n_own]]
            self.device_elite_indices = elite_index.astype(np.int64)
        last = self._n_iter - 1
        self._device_cem_finish(last, scores[last], context, host[3 + len(extra):n_own])
        self._t_since_replan = 0

    def _verbose_condition(self, cem_itr):
        if not self._hp.verbose:
            return False
        return bool(self._hp.verbose_every_iter or cem_itr == self._n_iter - 1)

    # ------------------------------------------------------------------ acting
    def _action_before_planning(self, t, state):
        """What to execute while t < start_planning: zeros, a fixed action, or weighted noise."""
        hp = self._hp
        if hp.zeros_for_start_frames:
            assert hp.hard_coded_start_action is None
            return np.zeros(self.agentparams['adim'])
        if hp.hard_coded_start_action:
            return np.array(hp.hard_coded_start_action)
        throwaway = hp.sampler(hp, self._adim, self._sdim)
        action = throwaway.sample_initial_actions(t, 1, state[-1])[0, 0] * hp.context_action_weight
        if hp.append_action:
            action = np.concatenate((action, hp.append_action), axis=0)
        return action

    def _replan_due(self):
        interval = self._hp.replan_interval
        return (not interval) or self._t_since_replan is None or self._t_since_replan + 1 >= interval

    def _action_from_plan(self, state, planned=False):
        """Replan when due, then read the next action off the best plan (``planned``: the caller has just run the due CEM
        call itself - ``BatchedPixelCostPlanner``)."""
        if not planned:
            if self._replan_due():
                self.perform_CEM(state)
            else:
                self._t_since_replan += 1
        return self._best_actions[0, self._t_since_replan]

    def act(self, t=None, i_tr=None, state=None):
        """One control step -> ``{'actions': [adim], 'plan_stat': {...}}``."""
        self._state, self.i_tr, self._t = state, i_tr, t
        if t < self._hp.start_planning:
            action = self._action_before_planning(t, state)
        else:
            action = self._action_from_plan(state)
        return self._finish_act(t, action)

    def _finish_act(self, t, action):
        assert action.shape == (self.agentparams['adim'],), "action shape does not match adim!"
        self._logger.log('time {}, action - {}'.format(t, action))

        remaining = None
        if self._best_actions is not None:      # tails of the elite plans, for samplers that reuse them
            first_unused = min(self._t_since_replan + 1, self._hp.T - 1)
            remaining = self._best_actions[:, first_unused:]
        self._sampler.log_best_action(action, remaining)
        return {'actions': action, 'plan_stat': self.plan_stat}
