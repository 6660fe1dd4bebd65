"""Counter-based folding proposal: the specification of ``vf_cem_sample_fold`` (``csrc/vf_cem.h``).

``PhiloxFoldingCEMSampler`` is to ``FoldingCEMSampler`` what ``PhiloxGaussianCEMSampler`` is to ``GaussianCEMSampler``: the
same families of plans from the same hyper-parameters, written so that a GPU kernel computes the very same numbers
(``tests/test_gpu_device_cem_folding.py``).  It is a complete host sampler in float64 NumPy and works with any predictor; with
a predictor that scores on the device the controller runs it there (``device_cem``).  Philox, the normals,
the fma, the factor fit, the draw and the elite order are ``philox_gaussian_sampler``'s and are not restated here.

Proposal
    ``mean [D]``, ``A [D, R]`` with ``sigma = A A^T``, ``D = nactions * 4``.  The first proposal of a planning call is
    ``A = diag(sqrt(diag(construct_initial_sigma)))`` around zero; a refit is ``fit_factor`` on the last representative of every
    held action of the K elites in ``(score, index)`` order - what ``vf_cem_refit`` computes.

Families by sample index, ``n = max(int(int(M * split_frac / 2) / 2), 1)``
    ``i < n``: ``TWO_PLACES``; ``n <= i < 2n``: ``ONE_PLACE``, whose last draw is held to the end of the plan; the rest: plain.

Counter ``(block, trial, sample i, call)``
    Nothing is rejected, so the trial word names the purpose of a draw.  Trial 0: the plain draw ``draw(mean, A, z)`` over all
    ``D`` dimensions - with the same key, call and sample the Gaussian twin's unrejected draw bit for bit.  Trial 1, block 0:
    the places, ``u_j = word_j / 2**32``; first place ``(u_0, u_1)``, second ``(u_2, u_3)``; ``ONE_PLACE`` uses ``(u_0, u_1)``.
    Trial ``2 + s``: the ``R`` normals of scripted step ``s``.

A scripted step
    ``v_c = m_c + g_c * y_c`` with ``y_c = sum_r A[c, r] z_r`` (one fma chain from 0.0, ``r`` ascending) over the rows
    ``c = 0..3`` of ``A``, the first action step's block (the reference's ``sigma[:4, :4]``).  ``g = (1, 1, 1, 1)`` on a carry,
    ``(sqrt(0.1), sqrt(0.1), 1, sqrt(0.5))`` on the spot, each a correctly rounded float64 constant.  ``m = (dx, dy, lift, 0)``
    with the carry ``(end - start) / repeat`` from the gripper's xy at the start of the call.  One product and one sum, each
    rounded once.  Steps past the script (``nactions > 5``) stay zero in ``TWO_PLACES`` and hold the last draw in ``ONE_PLACE``.

Post-processing
    Channels 0 - 2 are clipped to ``+-max_shift``, channel 3 is not; then every action is held ``repeat`` steps.  (The
    controller appends the ``append_action`` constants; the kernel writes them itself.)

Departures from ``FoldingCEMSampler``'s bits
    (a) Philox in place of the global NumPy stream.
    (b) The "narrow" covariance is ``G sigma G``, ``G = diag(g)``.  It equals the reference's for a diagonal ``sigma`` (every
        first proposal), and always on the xy block and the rotation variance; the reference leaves the cross terms unscaled,
        and that matrix need not be positive semi-definite.
    (c) The stream quirks of ``nactions >= 6`` (one draw lost, ``ValueError`` from 7) have no counterpart: a counter-based draw
        consumes nothing.  The values are the ones the reference's arrays end up with when it does not raise.
"""
import numpy as np

from .cem_sampler import CEMSampler
from .folding_sampler import FoldingCEMSampler, TWO_PLACES, ONE_PLACE, N_SCRIPTED
from .philox_gaussian_sampler import (philox4x32_10, standard_normals, fma64, fit_factor, draw, select_elites, _clip,
                                      MAX_D, MAX_K, MAX_WIDTH, MAX_SAMPLES)
from visual_foresight_amd.policy.utils.controller_utils import construct_initial_sigma

ADIM = 4
G_CARRY = np.ones(4)
G_SPOT = np.array([np.sqrt(0.1), np.sqrt(0.1), 1.0, np.sqrt(0.5)])
TRIAL_PLAIN, TRIAL_PLACES, TRIAL_STEP0 = 0, 1, 2


def n_scripted(M, split_frac):
    """Samples of each scripted family among ``M`` (the reference's halving, ``folding_sampler.py``)."""
    return max(int(int((M * split_frac) / 2) / 2), 1)


def places(key, call, samples):
    """The uniforms of trial 1, block 0 -> float64 ``[n, 4]``: first place ``(u_0, u_1)``, second ``(u_2, u_3)``."""
    samples = np.asarray(samples, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((samples.size, 4), dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = TRIAL_PLACES, samples, np.uint64(call)
    return philox4x32_10(ctr, key).astype(np.float64) / 4294967296.0


def step_of_action(script, nactions):
    """Per action step the scripted step whose draw it takes, -1: none (zero).  ``ONE_PLACE`` holds its last draw."""
    last = len(script) - 1
    hold = script is ONE_PLACE
    return np.array([a if a <= last else (last if hold else -1) for a in range(nactions)])


def step_means(script, ways):
    """``m [steps, n, 4]`` of a script: ``(dx, dy, lift, 0)`` with ``ways [n_ways, n, 2]`` the carries of every sample."""
    n = ways.shape[1]
    m = np.zeros((len(script), n, 4))
    for s, (way, lift) in enumerate(script):
        if way is not None:
            m[s, :, :2] = ways[way]
        m[s, :, 2] = lift
    return m


def scripted_step(A4, z, m, on_carry):
    """One scripted step of ``n`` samples: ``A4 [4, R]`` (the rows 0..3 of A), normals ``z [n, R]``, means ``m [n, 4]``."""
    y = np.zeros((z.shape[0], 4))
    for r in range(A4.shape[1]):
        y = fma64(A4[None, :, r], z[:, r, None], y)
    g = G_CARRY if on_carry else G_SPOT
    return m + g[None] * y


class PhiloxFoldingCEMSampler(CEMSampler):
    def __init__(self, hp, adim, sdim, **kwargs):
        super(PhiloxFoldingCEMSampler, self).__init__(hp, adim, sdim, **kwargs)
        if adim != ADIM:
            raise ValueError('PhiloxFoldingCEMSampler requires a base action dimension of 4, got %d' % adim)
        if hp.nactions < N_SCRIPTED:
            raise ValueError('PhiloxFoldingCEMSampler requires at least 5 action steps, got %d' % hp.nactions)
        self._D = hp.nactions * adim
        if self._D > MAX_D:
            raise ValueError('nactions * 4 = %d exceeds %d' % (self._D, MAX_D))
        if adim + len(hp.get('append_action') or ()) > MAX_WIDTH:
            raise ValueError('4 + len(append_action) exceeds %d' % MAX_WIDTH)
        if hp.get('num_samples', 3) > MAX_SAMPLES:
            raise ValueError('num_samples = %d exceeds %d' % (hp.num_samples, MAX_SAMPLES))
        if len(hp.max_shift) != 3:
            raise ValueError('max_shift holds the limits of x, y and z, got %r' % (hp.max_shift,))
        if hp.sampler_seed is None:
            self.key = (int(np.random.randint(2 ** 32)), int(np.random.randint(2 ** 32)))
        else:
            seed = int(hp.sampler_seed)
            self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self._call = 0                  # sampling calls so far: word 3 of the counter
        self._mean = self._A = None
        self._start_xy = np.zeros(2)    # where the carries start: xy of the gripper at the start of the planning call

    @staticmethod
    def get_default_hparams():
        hp = dict(FoldingCEMSampler.get_default_hparams())
        hp['sampler_seed'] = None       # Philox key; None: drawn from np.random at construction
        hp['device_cem'] = True         # run the CEM iterations on the GPU when the predictor can (False: host)
        return hp

    # ------------------------------------------------------------------ what the driver is told
    device_cem_driver = 'DeviceFoldingCEM'      # the class of device_cem.py that runs this sampler on the GPU

    def check_draws(self, M):
        """``n`` of a call that draws ``M`` sequences; the refusals of the family split."""
        if M % 3:
            raise ValueError('PhiloxFoldingCEMSampler splits the samples into settings with 3 means: %d is no multiple of 3' % M)
        n = n_scripted(M, self._hp.split_frac)
        if 2 * n > M:
            raise ValueError('split_frac = %r asks for 2 * %d scripted samples of %d' % (self._hp.split_frac, n, M))
        return n

    def device_draws(self, t, nsamples):
        """How many sequences every sampling call of a planning call at time ``t`` draws (known before it starts)."""
        self.check_draws(nsamples)
        return nsamples

    def next_call(self):
        """The counter word of the next sampling call; advances it."""
        c = self._call
        self._call += 1
        return c

    def initial_proposal(self, t, current_state=None):
        """``(mean [D], std [D])`` of the first proposal of a planning call at time ``t``; sets ``A = diag(std)`` and, given
        the state row the call starts from, the start of the carries."""
        std = np.sqrt(np.diag(construct_initial_sigma(self._hp, self._adim, t)))
        self._mean, self._A = np.zeros(self._D), np.diag(std)
        if current_state is not None:
            self._start_xy = np.array(current_state[:2], dtype=np.float64)
        return self._mean, std

    def start_xy(self):
        return self._start_xy

    # ------------------------------------------------------------------ proposals
    def sample_initial_actions(self, t, nsamples, current_state):
        self.initial_proposal(t, current_state)
        return self._sample(nsamples)

    def elite_rows(self, actions):
        """Elite plans ``[K, T, >= 4]`` -> ``[K, D]``: the last representative of every held action."""
        hp = self._hp
        a = np.asarray(actions, dtype=np.float64)[:, :, :self._adim]
        return a.reshape(-1, hp.nactions, hp.repeat, self._adim)[:, :, -1, :].reshape(-1, self._D)

    def refit(self, best_actions):
        self._mean, self._A = fit_factor(self.elite_rows(best_actions))

    def sample_next_actions(self, n_samples, best_actions, scores):
        self.refit(best_actions)
        return self._sample(n_samples)

    select_elites = staticmethod(select_elites)

    # ------------------------------------------------------------------ internals
    def _scripted(self, script, samples, ways, call):
        """The plans ``[n, nactions, 4]`` of ``samples`` under ``script``; ``ways [n_ways, n, 2]``."""
        R = self._A.shape[1]
        means = step_means(script, ways)
        out = np.zeros((samples.size, self._hp.nactions, 4))
        takes = step_of_action(script, self._hp.nactions)
        for s, (way, _) in enumerate(script):
            z = standard_normals(self.key, call, samples, TRIAL_STEP0 + s, R)
            out[:, takes == s] = scripted_step(self._A[:4], z, means[s], way is not None)[:, None]
        return out

    def _carry(self, start, end):
        return (end - start) / self._hp.repeat

    def _sample(self, M):
        hp = self._hp
        n = self.check_draws(M)
        call = self.next_call()
        actions = np.zeros((M, hp.nactions, self._adim))
        start = self._start_xy[None]

        two = np.arange(n)
        u = places(self.key, call, two)
        first, second = u[:, :2], u[:, 2:]
        actions[:n] = self._scripted(TWO_PLACES, two, np.stack((self._carry(start, first), self._carry(first, second))), call)
        one = np.arange(n, 2 * n)
        place = places(self.key, call, one)[:, :2]
        actions[n:2 * n] = self._scripted(ONE_PLACE, one, self._carry(start, place)[None], call)

        plain = np.arange(2 * n, M)
        if plain.size:
            x = draw(self._mean, self._A, standard_normals(self.key, call, plain, TRIAL_PLAIN, self._A.shape[1]))
            actions[2 * n:] = x.reshape(plain.size, hp.nactions, self._adim)

        limit = np.asarray(hp.max_shift, dtype=np.float64)
        actions[:, :, :3] = _clip(actions[:, :, :3], -limit, limit)
        return np.repeat(actions, hp.repeat, axis=1)
