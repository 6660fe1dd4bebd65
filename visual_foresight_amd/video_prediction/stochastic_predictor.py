"""Latent-conditioned (stochastic) rollouts on top of the HIP predictor.

BASELINE config 5 asks for a stochastic predictor evaluated with several latent draws per action
sequence ("n_latent = 5 z-draws ~ N(0, I) per action ... latent draws fold into
the sample axis; per-action cost = mean over its draws").  The SAVP architecture is external to
the reference (``visual_mpc/video_prediction/vpred_model_interface.py:52-58`` only instantiates
it); the generator this repo implements for it is specified in ``savp_arch.py`` (``arch='savp'``, the
default here: four scales, first-frame compositing, per-step latent; parity unpinned) and
``arch='cdna'`` conditions the plain CDNA network of ``cdna_arch.py`` the same way.  In both, the latent
``z_t`` enters exactly where the action does (tiled and concatenated at the bottleneck, enc3), i.e. the
engine is built for ``adim + zdim`` "action" channels.

Every action sequence is rolled ``n_latent`` times with common random numbers (draw ``d`` uses the
same ``z[d, t]`` for every action, redrawn per planning call from ``latent_seed``), which keeps the
comparison between candidates low-variance; the reference's vestigial hook repeats each action
``stochastic_planning[0]`` times (``samplers/gaussian_sampler.py:140-141``).  The draws of one
action are consecutive rows of the rolled batch, the engine averages their costs on the device
(``vf_config.n_draws``), so one score row per ACTION leaves the GPU and the all-gather and the
propagation fetch work exactly as for the deterministic predictor (sharded by action, owner rank
exports, all-reduce).

``PhiloxStochasticHipPredictor`` is the same predictor with a counter-based latent stream (``philox_latents``) in place of
``np.random.RandomState``: a GPU kernel can compute those numbers, so on one engine it draws and folds the latents on the
device (``vf_cem_latents`` / ``vf_cem_fold_latents``, ``csrc/vf_cem.h``) and offers the ``score*_device`` entries of the
device-resident CEM route.  Opt-in: ``StochasticHipPredictor`` and its stream stay as they are.
"""
import contextlib

import numpy as np

from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation

LATENT_TRIAL = 0xFFFFFFFF       # the trial word of the latents' counters: no sampler draws under it


def philox_latents(seed, call, n_latent, T, zdim):
    """The latents of scoring call ``call`` under ``seed`` -> float64 ``[n_latent, T, zdim]``: the specification of
    ``vf_cem_latents``.  ``z[d, t, j]`` is normal ``t * zdim + j`` of ``philox_gaussian_sampler.standard_normals`` with sample
    word ``d``, call word ``call & 0xFFFFFFFF`` and trial word ``LATENT_TRIAL`` under the key ``(seed & 0xFFFFFFFF,
    (seed >> 32) & 0xFFFFFFFF)``.  The trial word keeps the latents off every sampler's counters when ``latent_seed ==
    sampler_seed``: the Gaussian sampler draws under trials ``< max_trials``, the folding sampler ``2 + s``, the correlated
    sampler 0."""
    from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import standard_normals
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    z = standard_normals(key, int(call) & 0xFFFFFFFF, np.arange(int(n_latent)), LATENT_TRIAL, int(T) * int(zdim))
    return np.ascontiguousarray(z).reshape(int(n_latent), int(T), int(zdim))


def fold_latents(actions, z):
    """``actions [M, T, width]``, ``z [n_latent, T, zdim]`` -> ``[M * n_latent, T, width + zdim]``, draw-minor: row
    ``a * n_latent + d`` is ``[actions[a], z[d]]`` (common random numbers across actions).  The specification of
    ``vf_cem_fold_latents`` and the layout of ``StochasticHipPredictor._prepare``."""
    actions, z = np.asarray(actions), np.asarray(z)
    M, n_latent = actions.shape[0], z.shape[0]
    out = np.empty((M * n_latent, actions.shape[1], actions.shape[2] + z.shape[2]), dtype=np.result_type(actions, z))
    rows = out.reshape(M, n_latent, actions.shape[1], -1)
    rows[..., :actions.shape[2]] = actions[:, None]
    rows[..., actions.shape[2]:] = z[None]
    return out


class StochasticHipPredictor(HipVPredEvaluation):
    options = {}            # class-level defaults, see with_options()

    @classmethod
    def with_options(cls, **options):
        """A subclass with n_latent / zdim / latent_seed baked in, for use as ``predictor_class`` (the
        controller's hyper-parameter set stays exactly the reference's)."""
        return type(cls.__name__, (cls,), {'options': dict(cls.options, **options)})

    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        hp = dict(self.options, **hparams)
        self.n_latent = int(hp.pop('n_latent', 5))
        self.zdim = int(hp.pop('zdim', 8))
        self.latent_seed = int(hp.pop('latent_seed', 0))
        self.adim = int(hp.get('adim', 4))
        self._calls = 0
        self._z = None
        inner = dict(hp, adim=self.adim + self.zdim, n_draws=self.n_latent, arch=hp.get('arch', 'savp'), zdim=self.zdim)
        super(StochasticHipPredictor, self).__init__(model_path, inner, n_gpus=n_gpus, first_gpu=first_gpu)

    def draw_latents(self, T):
        """z[n_latent, T, zdim] for this planning call (deterministic in latent_seed and call count)."""
        rs = np.random.RandomState(self.latent_seed + self._calls)
        return rs.normal(0.0, 1.0, (self.n_latent, T, self.zdim))

    def _adim_in(self):
        return self.adim

    def _prepare(self, context, actions):
        """Fold the latent draws into the sample axis, draw-minor: row ``a * n_latent + d`` = action a, draw d."""
        actions = np.asarray(actions, dtype=np.float64)
        n, T = actions.shape[:2]
        z = self._z if self._z is not None else self.draw_latents(T)
        tiled = np.repeat(actions, self.n_latent, axis=0)                                   # [n*nl, T, adim]
        zz = np.tile(z, (n, 1, 1))
        ctx_actions = np.asarray(context['context_actions'], dtype=np.float64).reshape(-1, self.adim)
        ctx = dict(context, context_actions=np.concatenate(
            [ctx_actions, np.zeros((ctx_actions.shape[0], self.zdim))], axis=1))
        return ctx, np.concatenate([tiled, zz], axis=2)

    @contextlib.contextmanager
    def _scoring_call(self, actions):
        """One set of draws per scoring call (``score``, ``score_goal_image``, ``score_frames``), shared by every rank and
        lane; the call counts whether or not it is refused afterwards.  ``__call__`` draws for itself and does not count."""
        self._z = self.draw_latents(np.asarray(actions).shape[1])
        self._calls += 1
        try:
            yield
        finally:
            self._z = None


class PhiloxStochasticHipPredictor(StochasticHipPredictor):
    """``StochasticHipPredictor`` whose latents are ``philox_latents(latent_seed, call, ...)``.  On the host route it is a
    complete predictor through the inherited ``_prepare`` (lanes and ranks included).  On one engine the ``score*_device``
    entries draw the call's latents and fold them into the device candidates there; ``last_latents_dev`` keeps the float32
    latents ``[n_latent, T, zdim]`` of the last such call (each the float64 normal rounded once, within 1 float32 ulp of
    the specification: the device's ``log`` / ``sin`` / ``cos``)."""
    last_latents_dev = None

    def draw_latents(self, T):
        return philox_latents(self.latent_seed, self._calls, self.n_latent, T, self.zdim)

    def _prepare_device(self, context, actions_dev):
        """The device twin of ``_prepare``: the call's latents and the folded sequences ``[M * n_latent, T, adim + zdim]`` as
        device tensors, the context actions padded with ``zdim`` zeros.  Consumes one call number, as ``_scoring_call``
        does for a host entry.  Only enqueues."""
        torch, lib = self._torch, self._libh
        M, T, width = (int(v) for v in actions_dev.shape)
        z = torch.empty((self.n_latent, T, self.zdim), dtype=torch.float32, device=self.device)
        seqs = torch.empty((M * self.n_latent, T, width + self.zdim), dtype=torch.float32, device=self.device)
        seed = self.latent_seed
        _lib.check(lib.vf_cem_latents(self.device.index, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                      self._calls & 0xFFFFFFFF, self.n_latent, T, self.zdim, z.data_ptr(), self._stream()))
        self._calls += 1
        _lib.check(lib.vf_cem_fold_latents(self.device.index, actions_dev.data_ptr(), z.data_ptr(), M, self.n_latent, T,
                                           width, self.zdim, seqs.data_ptr(), self._stream()))
        self.last_latents_dev = z
        ctx_actions = np.asarray(context['context_actions'], dtype=np.float64).reshape(-1, self.adim)
        ctx = dict(context, context_actions=np.concatenate(
            [ctx_actions, np.zeros((ctx_actions.shape[0], self.zdim))], axis=1))
        return ctx, seqs
