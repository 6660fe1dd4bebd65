"""Counter-based time-correlated noise proposal: the specification of the device-resident CEM iteration of the RoboNet-era
experiments.

``PhiloxCorrelatedNoiseSampler`` proposes as ``CorrelatedNoiseSampler`` does (same hyper-parameters and defaults, the same
AR(1) filter with its wrap-around first step, the same soft-mean refit) but is written so that a GPU kernel can compute the
very same numbers: ``cem_soft_refit_kernel`` / ``cem_sample_corr_kernel`` of ``csrc/vf_cem.h`` are held to this file
(``tests/test_gpu_device_cem_correlated.py``).  It is a complete host sampler in float64 NumPy and works with any predictor;
with ``HipVPredEvaluation`` the controller runs it on the device (``device_cem``).  Two things differ from
``CorrelatedNoiseSampler``'s bits: the random numbers (Philox, not ``np.random``) and, with ``refit_cov``, the colouring,
which is kept in factor form.

Random numbers
    Philox4x32-10 and Box-Muller exactly as in ``philox_gaussian_sampler.py`` (same key rule).  The white normal of sample
    ``i`` at flat index ``d = a * adim + c`` in sampling call ``call`` is element ``d`` of
    ``standard_normals(key, call, i, 0, D)``: the trial word is always 0, there is no rejection.

Shaping (every operation rounded on its own)
    Without a fitted covariance ``s_d = w_d * std_c + bias_c`` (bias 0.0 when ``mean_bias`` is None).  With ``refit_cov``
    after a refit the covariance stays in the factor form ``A[d, k] = (e_kd - m_d) / sqrt(K - 1)`` of ``fit_factor`` and the
    reference's ``white @ cov`` is ``(white @ A) @ A^T``: two fma chains from 0.0, ``y_k = sum_d w_d A[d, k]`` (d ascending),
    then ``s_d = sum_k A[d, k] y_k`` (k ascending); no bias, as in the reference.  No ``D x D`` matrix is formed.

AR(1)
    Per sample and column, ``o_a = (beta_0 * s_a) + (beta_1 * prev)``: two rounded products, one rounded sum.  ``prev`` is
    ``o_{a-1}``; for ``a = 0`` the unfiltered ``s_{nactions-1}``, or - with ``smooth_across_last_action`` and a logged
    action - the first ``adim`` entries of the last chosen action.

Refit
    Elites ``[K, D]`` in ``select_elites`` order.  ``g_k = -score_k``, ``soft_k = exp(kappa * (g_k - g_0))``,
    ``num_d = sum_k (e_kd * soft_k)`` (k ascending, product and sum rounded), ``den = sum_k soft_k`` then ``+ 1e-4``,
    ``centre_d = num_d / den``.

Candidates
    The first proposal of a planning call is ``o`` itself (nothing is added: signed zeros survive), later ones
    ``o_d + centre_d``; ``[M, nactions, adim]``.
"""
import numpy as np

from .cem_sampler import CEMSampler
from .correlated_noise import DEFAULTS
from .philox_gaussian_sampler import (philox4x32_10, standard_normals, fma64, select_elites, fit_factor,  # noqa: F401
                                      MAX_D, MAX_K, MAX_WIDTH, MAX_SAMPLES)


def soft_refit(flat, scores, kappa):
    """Elites ``[K, D]`` in rank order and their scores -> ``(soft [K], centre [D])``."""
    flat = np.asarray(flat, dtype=np.float64)
    gain = -np.asarray(scores, dtype=np.float64).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        soft = np.exp(kappa * (gain - gain[0]))
        num, den = np.zeros(flat.shape[1]), 0.0
        for k in range(flat.shape[0]):
            num = num + flat[k] * soft[k]
            den = den + soft[k]
        return soft, num / (den + 1e-4)


def colour(A, w):
    """``(w A) A^T`` of the white normals ``w [n, D]`` under the factor ``A [D, K]``: two fma chains from 0.0."""
    y = np.zeros((w.shape[0], A.shape[1]))
    for d in range(A.shape[0]):
        y = fma64(w[:, d, None], A[None, d, :], y)
    s = np.zeros(w.shape)
    for k in range(A.shape[1]):
        s = fma64(A[None, :, k], y[:, k, None], s)
    return s


class PhiloxCorrelatedNoiseSampler(CEMSampler):
    def __init__(self, hp, adim, sdim, **kwargs):
        super(PhiloxCorrelatedNoiseSampler, self).__init__(hp, adim, sdim, **kwargs)
        self._adim = len(hp.initial_std)        # the std list, not the agent, fixes the action dimension
        self._D = int(hp.nactions) * self._adim
        n_tail = len(hp.get('append_action') or ())
        if not 1 <= self._D <= MAX_D:
            raise ValueError('nactions * adim = %d outside 1..%d' % (self._D, MAX_D))
        if self._adim + n_tail > MAX_WIDTH:
            raise ValueError('adim + len(append_action) = %d exceeds %d' % (self._adim + n_tail, MAX_WIDTH))
        if hp.get('num_samples', 1) > MAX_SAMPLES:
            raise ValueError('num_samples = %d exceeds %d' % (hp.num_samples, MAX_SAMPLES))
        if hp.mean_bias is not None and len(hp.mean_bias) != self._adim:
            raise ValueError('mean_bias has %d entries, initial_std %d' % (len(hp.mean_bias), self._adim))
        if hp.sampler_seed is None:
            self.key = (int(np.random.randint(2 ** 32)), int(np.random.randint(2 ** 32)))
        else:
            seed = int(hp.sampler_seed)
            self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self._call = 0                  # sampling calls so far: word 3 of the counter
        self._centre = self._A = None   # None: the first proposal of a planning call
        self.last_soft = None           # the elites' weights of the last refit
        self.last_centre = None         # its soft mean [D]
        self.last_mean = None           # with refit_cov: the elites' plain mean [D] (A is about it)

    @staticmethod
    def get_default_hparams():
        return dict(DEFAULTS, sampler_seed=None,        # Philox key; None: drawn from np.random at construction
                    device_cem=True)                    # run the CEM iterations on the GPU when the predictor can

    # ------------------------------------------------------------------ what the controller and the kernels are told
    device_cem_driver = 'DeviceCorrelatedCEM'           # the class of device_cem.py that runs this sampler on the GPU

    def device_draws(self, t, nsamples):
        """How many sequences every sampling call of a planning call at time ``t`` draws."""
        return nsamples

    def std(self):
        return np.asarray(self._hp.initial_std, dtype=np.float64)

    def bias(self):
        hp = self._hp
        return np.zeros(self._adim) if hp.mean_bias is None else np.asarray(hp.mean_bias, dtype=np.float64)

    def first_predecessor(self):
        """``[adim]`` the filter's first step is smoothed against, or None for the wrap-around to the last noise step."""
        if self._hp.smooth_across_last_action and len(self._chosen_actions):
            return np.asarray(self._chosen_actions[-1], dtype=np.float64)[:self._adim].copy()
        return None

    def next_call(self):
        """The counter word of the next sampling call; advances it."""
        c = self._call
        self._call += 1
        return c

    select_elites = staticmethod(select_elites)

    # ------------------------------------------------------------------ proposals
    def start_planning_call(self):
        """Forget the fit: the next sampling call draws the first proposal."""
        self._centre = self._A = None

    def sample_initial_actions(self, t, nsamples, current_state):
        self.start_planning_call()
        return self._sample(nsamples)

    def refit(self, best_actions, scores):
        flat = np.asarray(best_actions, dtype=np.float64)[:, :, :self._adim].reshape(-1, self._D)
        self.last_soft, self._centre = soft_refit(flat, scores, self._hp.kappa)
        self.last_centre = self._centre
        if self._hp.refit_cov:
            self.last_mean, self._A = fit_factor(flat)

    def sample_next_actions(self, n_samples, best_actions, scores):
        self.refit(best_actions, scores)
        return self._sample(n_samples)

    # ------------------------------------------------------------------ internals
    def shape(self, white):
        """White normals ``[n, D]`` -> shaped noise ``[n, D]``."""
        if self._A is not None:
            return colour(self._A, white)
        return white * np.tile(self.std(), self._hp.nactions)[None] + np.tile(self.bias(), self._hp.nactions)[None]

    def ar1(self, noise):
        """``[n, nactions, adim]`` -> the filtered sequences."""
        b0, b1 = self._hp.beta_0, self._hp.beta_1
        out = noise.copy()
        first = self.first_predecessor()
        prev = noise[:, -1, :] if first is None else first[None]
        for a in range(self._hp.nactions):
            out[:, a, :] = b0 * noise[:, a, :] + b1 * prev
            prev = out[:, a, :]
        return out

    def _sample(self, M):
        call = self.next_call()
        white = standard_normals(self.key, call, np.arange(M), 0, self._D)
        out = self.ar1(self.shape(white).reshape(M, self._hp.nactions, self._adim))
        if self._centre is None:
            return out
        return out + self._centre.reshape(1, self._hp.nactions, self._adim)
