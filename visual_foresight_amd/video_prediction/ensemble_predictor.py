"""Ensemble of independently trained predictors scored as mean + variance (uncertainty-aware planning).

The reference's ``CEM_Controller_Ensemble_Vidpred``
(``visual_mpc/policy/cem_controllers/variants/ensemble_vidpred.py:32-61``) rolls every candidate action sequence through
``num_ensembles`` networks and, per step, replaces the expected pixel distance by the member mean plus
``lambda_variance`` times the member variance: sequences the members disagree about cost more, so the elite argsort
cannot exploit one model's error.

Here the members are E engines of ONE ``vf_config`` (``HipVPredEvaluation``, or ``StochasticHipPredictor`` for the
SAVP-class archs or when ``n_latent`` is given) on one device, driven from one stream.  ``score()`` prepares the
sequences once (the latent draws are shared: draw d is the same z for every member), then per chunk every member runs
``vf_rollout`` on the same sequences and one ``vf_ensemble_scores`` call reduces the E members' resident cost sums to
the ensemble scores on the device - no predicted video leaves the GPU.

Multi-GPU: under ``torch.distributed`` every rank holds all E members on its own GPU, scores its action shard and the
score rows are all-gathered unchanged.  In-process lanes (``n_gpus > 1`` without ``torch.distributed``) are refused.

``score_device`` is ``score`` without the gather, for the device-resident CEM route: the members roll
device candidates as they lie there.  Stochastic members need the counter-based latent stream for it (the member option
``philox_latents=True`` selects ``PhiloxStochasticHipPredictor``; member 0 draws and folds once for all members).
"""
import ctypes
import os

import numpy as np

from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation, pixel_cost_columns, score_rows
from visual_foresight_amd.video_prediction.sharding import dist_info as _dist_info
from visual_foresight_amd.video_prediction.stochastic_predictor import PhiloxStochasticHipPredictor, StochasticHipPredictor


class EnsembleHipPredictor(object):
    wants_agent_params = True
    supports_task_weights = True
    n_context_default = 2
    options = {}            # class-level defaults, see with_options()

    @classmethod
    def with_options(cls, **options):
        """A subclass with num_ensembles / lambda_variance (and member options such as arch, n_latent) baked in, for use
        as ``predictor_class``."""
        return type(cls.__name__, (cls,), {'options': dict(cls.options, **options)})

    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        import torch
        self._torch = torch
        hp = dict(self.options, **hparams)
        self.num_ensembles = int(hp.pop('num_ensembles', 4))
        self.lambda_variance = float(hp.pop('lambda_variance', 0.1))
        if not 1 <= self.num_ensembles <= 16:
            raise ValueError('num_ensembles must be 1..16, got %d' % self.num_ensembles)
        if _dist_info()[1] == 1 and int(n_gpus) > 1:
            raise ValueError('EnsembleHipPredictor has no in-process multi-GPU lanes (n_gpus=%d): run one rank per GPU '
                             'under torch.distributed instead' % int(n_gpus))
        from visual_foresight_amd.video_prediction.hip_predictor import designated_pixel_count_of
        if designated_pixel_count_of(hp) == 0:      # (before a member engine is built)
            raise ValueError('EnsembleHipPredictor combines the members\' pixel-cost sums: its members cannot be frames-only '
                             '(designated_pixel_count 0 / no_pix_distrib)')
        stochastic = hp.pop('stochastic', None)
        if stochastic is None:
            stochastic = 'n_latent' in hp or hp.get('arch', 'cdna') != 'cdna'
        philox = bool(hp.pop('philox_latents', False))       # the latent stream the device entries can draw
        if philox and not stochastic:
            raise ValueError('philox_latents selects the latent stream of stochastic members: these members draw none')
        member_cls = (PhiloxStochasticHipPredictor if philox else StochasticHipPredictor) if stochastic else HipVPredEvaluation
        self.model_path = model_path
        seed = int(hp.get('seed', 0))
        self.members = [member_cls('', dict(hp, seed=seed + 1000 * m), n_gpus=n_gpus, first_gpu=first_gpu)
                        for m in range(self.num_ensembles)]
        m0 = self.members[0]
        for name in ('n_context', 'sequence_length', 'n_cam', 'n_draws', 'run_batch_size', 'cfg', 'arch', 'device',
                     'device_index'):
            setattr(self, name, getattr(m0, name))
        self.weights = None
        self.last_cost_per_step = None
        self.last_cost_rows_dev = None      # score_device: [M, score | per task | per task x step] on the device
        self._last_prepared = None

    # ------------------------------------------------------------------ weights
    def _member_path(self, m):
        if isinstance(self.model_path, (list, tuple)):
            return os.path.expanduser(self.model_path[m])
        if not self.model_path:
            return ''
        path = os.path.join(os.path.expanduser(self.model_path), 'member%d' % m)
        if not os.path.isdir(path):
            raise ValueError('ensemble checkpoint %s has no member%d/ directory' % (self.model_path, m))
        return path

    def restore(self, weights=None):
        """Load ``member%d/`` sub-directories of ``model_path`` or a list of E paths (each may hold ``view%d/``) or, without
        a path, seeded random weights (member m: ``seed + 1000 * m + view``).  ``weights``: E weight sets (each one
        ``CdnaWeights`` or a list per view)."""
        if weights is None:
            if isinstance(self.model_path, (list, tuple)) and len(self.model_path) != self.num_ensembles:
                raise ValueError('need one path per member (%d), got %d' % (self.num_ensembles, len(self.model_path)))
            for m, member in enumerate(self.members):
                member.model_path = self._member_path(m)
                member.restore()
        else:
            if len(weights) != self.num_ensembles:
                raise ValueError('need one weight set per member (%d), got %d' % (self.num_ensembles, len(weights)))
            for member, w in zip(self.members, weights):
                member.restore(w)
        self.weights = [m.weights for m in self.members]
        return self

    # ------------------------------------------------------------------ scoring
    def _prepare(self, context, actions):
        """The sequences every member rolls, prepared once (a stochastic member 0 draws the call's latents)."""
        m0 = self.members[0]
        with m0._scoring_call(actions):
            return m0._prepare(context, actions)

    def _adim_in(self):
        return self.members[0]._adim_in()

    def score_device_refusal(self):
        """Why ``score_device`` cannot serve the ensemble, or None when it can: the members' own refusals
        (``HipVPredEvaluation.score_device_refusal``: ranks, sequences prepared on the host)."""
        m0 = self.members[0]
        if m0._prepares_on_host():
            return 'score_device rolls the actions as they lie on the device: the ensemble prepares its sequences on the host'
        return m0.score_device_refusal()

    def _member_rows(self, prepared, local, n, lo, goal_pix, finalweight, task_weights):
        """Every member rolls the device sequences ``local [n * n_draws, T, engine adim]`` (actions ``[lo, lo + n)`` of the
        call ``prepared = (context, sequences, M)``), chunk by chunk, and ``vf_ensemble_scores`` reduces each chunk -> device
        float64 rows ``[n, score | per task | per task x step]``.  Only enqueues (the context upload aside)."""
        torch = self._torch
        m0 = self.members[0]
        T = self.sequence_length - self.n_context
        ntask = self.n_cam * self.cfg.ndesig
        nd = self.n_draws
        tw = m0._task_weights_c(task_weights)
        handles = (ctypes.c_void_p * self.num_ensembles)(*[m._handle.value for m in self.members])
        for member in self.members:
            member._last_prepared = prepared
            member._set_context(prepared[0])
        rows = torch.empty((n, 1 + ntask + ntask * T), dtype=torch.float64, device=self.device)
        scores, per_task, cps = rows[:, 0], rows[:, 1:1 + ntask], rows[:, 1 + ntask:]
        bs = self.run_batch_size // nd
        own_s = torch.empty(bs, dtype=torch.float64, device=self.device)
        own_pt = torch.empty((bs, ntask), dtype=torch.float64, device=self.device)
        c_s = torch.empty(bs, dtype=torch.float64, device=self.device)
        c_pt = torch.empty((bs, ntask), dtype=torch.float64, device=self.device)
        c_cps = torch.empty((bs, ntask * T), dtype=torch.float64, device=self.device)
        for c0 in range(0, n, bs):
            c1 = min(c0 + bs, n)
            for member in self.members:
                member._rollout_chunk(local[c0 * nd:c1 * nd], goal_pix, finalweight, own_s[:c1 - c0],
                                      own_pt[:c1 - c0], task_weights)
                member._last_lo, member._last_M = lo + c0, c1 - c0
            _lib.check(m0._libh.vf_ensemble_scores(handles, self.num_ensembles, ctypes.c_float(self.lambda_variance),
                                                   ctypes.c_float(finalweight), tw, c_s.data_ptr(), c_pt.data_ptr(),
                                                   c_cps.data_ptr(), m0._stream()))
            scores[c0:c1], per_task[c0:c1], cps[c0:c1] = c_s[:c1 - c0], c_pt[:c1 - c0], c_cps[:c1 - c0]
        return rows

    def score_device(self, context, actions_dev, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
        """``score`` without the gather: every member rolls ``actions_dev`` - a contiguous float32 tensor ``[M, T, adim]`` on
        the members' device - and the device float64 ensemble ``scores [M]`` come back.  Only enqueues (the context upload
        aside, when it changed); the caller checks the downloaded scores with ``_check_scores``.  Chunked by
        ``run_batch_size`` like ``score``; every member keeps its last chunk resident, and ``actions_dev`` must stay untouched
        for as long as ``fetch_pixel_distributions`` may be asked.  With stochastic members, member 0 draws and folds the
        call's latents once for all (one call number, as in ``score``).  The whole rows stay in ``last_cost_rows_dev``
        ``[M, score | per task | per task x step]``.  ValueError: ``score_device_refusal``."""
        reason = self.score_device_refusal()
        if reason:
            raise ValueError(reason)
        torch = self._torch
        m0 = self.members[0]
        M = m0._check_actions_dev(actions_dev)
        with torch.cuda.device(self.device):
            ctx_p, seqs = m0._prepare_device(context, actions_dev)
            self._last_prepared = (ctx_p, seqs, M)
            rows = self._member_rows(self._last_prepared, seqs, M, 0, goal_pix, finalweight, task_weights)
            self.last_cost_rows_dev = rows
            # (only_take_first_view: task 0 alone is the score, pixel_cost_columns)
            return rows[:, 1 if only_take_first_view else 0].contiguous()

    def split_cost_rows(self, rows_np):
        """Host rows of the ensemble cost -> (scores [M], per task [M, ncam*nd], cost per step [M, ncam*nd, T])."""
        ntask = self.n_cam * self.cfg.ndesig
        M = rows_np.shape[0]
        return (np.ascontiguousarray(rows_np[:, 0]), np.ascontiguousarray(rows_np[:, 1:1 + ntask]),
                np.ascontiguousarray(rows_np[:, 1 + ntask:]).reshape(M, ntask, -1))

    def score(self, context, inputs, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
        """Ensemble cost of every action: (scores[M], scores_per_task[M, ncam*nd]) float64, as
        ``HipVPredEvaluation.score``.  ``last_cost_per_step`` [M, ncam*nd, T] holds the per-step ensemble cost
        (mean + lambda * variance, averaged over latent draws)."""
        torch = self._torch
        m0 = self.members[0]
        actions = m0._check_actions(inputs['actions'])
        M = actions.shape[0]
        T = self.sequence_length - self.n_context
        ntask = self.n_cam * self.cfg.ndesig
        ctx_p, seqs = self._prepare(context, actions)
        self._last_prepared = (ctx_p, seqs, M)

        def rows_of(_, share, n, lo):       # [score | per task | per task x step]; the engines are the members
            local = torch.from_numpy(np.ascontiguousarray(share, dtype=np.float32)).to(self.device)
            return self._member_rows((ctx_p, seqs, M), local, n, lo, goal_pix, finalweight, task_weights)

        rows_np = score_rows(self, seqs, M, 1 + ntask + ntask * T, rows_of)
        self.last_cost_per_step = np.ascontiguousarray(rows_np[:, 1 + ntask:]).reshape(M, ntask, T)
        return pixel_cost_columns(rows_np[:, :1 + ntask], only_take_first_view)

    def _check_scores(self, scores_np):
        if np.isnan(scores_np).any():
            status = 0
            for member in self.members:
                member._ctx_key = None      # the engine dropped its context-only cache with the status
                status = max(status, member.device_status())
            raise _lib.VfError('a member\'s persistent rollout reported a failure (device status %d): scores are '
                               'invalid' % status)

    def device_status(self):
        return max(m.device_status() for m in self.members)

    def fetch_pixel_distributions(self, sample_index):
        """Member mean of the normalised distributions ``[T, ncam, H, W, ndesig]`` of one action of the last
        ``score()`` call (its first latent draw)."""
        acc = None
        for member in self.members:
            d = member.fetch_pixel_distributions(sample_index).astype(np.float64)
            acc = d if acc is None else acc + d
        return (acc / self.num_ensembles).astype(np.float32)

    def __call__(self, context, inputs):
        """Reference keys as member means, plus ``ensemble_pixel_distributions`` [E, M, T, ncam, H, W, nd] for host
        scoring (with latent draws, the first draw of every action)."""
        m0 = self.members[0]
        actions = m0._check_actions(inputs['actions'])
        M = actions.shape[0]
        ctx_p, seqs = self._prepare(context, actions)
        self._last_prepared = (ctx_p, seqs, M)
        outs = []
        for member in self.members:
            member._last_prepared = (ctx_p, seqs, M)
            outs.append(member._materialise(ctx_p, seqs, M, 0))
        res = {k: (sum(o[k].astype(np.float64) for o in outs) / self.num_ensembles).astype(np.float32)
               for k in outs[0]}
        res['ensemble_pixel_distributions'] = np.stack([o['predicted_pixel_distributions'] for o in outs])
        return res
