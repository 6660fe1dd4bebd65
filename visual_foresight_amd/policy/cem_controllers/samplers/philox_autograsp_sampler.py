"""Counter-based autograsp proposal: the specification of ``vf_cem_sample_autograsp`` (``csrc/vf_cem.h``, fifth part).

``PhiloxAutograspSampler`` is to ``AutograspSampler`` what ``PhiloxGaussianCEMSampler`` is to ``GaussianCEMSampler``: a Gaussian
proposal over the first ``adim - 1`` channels (the moves) whose last channel, the gripper command, is derived - written so that
a GPU kernel computes the very same numbers (``tests/test_gpu_device_cem_autograsp.py``).  It is a complete host sampler in
float64 NumPy and works with any predictor; with a predictor that scores on the device the controller runs it there
(``device_cem``).  Philox, the normals, the draw, rejection, the factor fit and the elite order are
``philox_gaussian_sampler``'s and are not restated here.

Moves
    Columns ``0 .. adim - 2`` are exactly what a ``PhiloxGaussianCEMSampler(hp, adim - 1, sdim)`` with the same key and call
    number draws: the counters ``(block, trial n, sample i, call)``, rejection, discretisation, truncation, ``repeat``,
    ``add_zero_action``, ``reuse_mean`` and the refit on the elites' first ``adim - 1`` columns.

Gripper by height (``gripper_from_moves``)
    The first proposal of every planning call, and every refit when ``no_refit`` is true.  A pure function of the moves
    ROUNDED TO FLOAT32 - what a predictor is fed and what a kernel stores.  Per sample, with ``z32_t`` the lift (channel 2)
    of step ``t``: ``p_t = float64(z32_t) * action_norm_factor``; ``c_0 = p_0``, ``c_t = c_{t-1} + p_t`` sequentially over the
    ``T = nactions * repeat`` steps; ``h_t = c_t + state_z``; ``shut_t = h_t < z_thresh``; every operation rounded once, in
    this order (``np.cumsum(...) + current_state[2]`` of the reference).  Unless ``reopen`` the gripper stays shut from the
    first shut step on.  With ``deviation_prob > 0`` step ``t`` is then flipped when ``u_t < deviation_prob``.

Uniforms (``grip_uniforms``)
    ``u_t = word (t % 4) / 2**32`` of the Philox counter ``(block t // 4, trial 0xFFFFFFFE, sample i, call)``.  No sampler uses
    that trial word: the Gaussian trials stay below ``max_trials`` (the constructor refuses ``max_trials >= 0xFFFFFFFE``), the
    folding sampler uses 1 .. 6, the latent draws ``0xFFFFFFFF``.  ``deviation_prob`` 0 draws none.

Gripper by the elites' share (``gripper_from_share``)
    Refits with ``no_refit`` false.  ``count_t`` = the elites whose gripper value at step ``t`` equals
    ``float32(gripper_close_cmd)``; ``share_t = float32(count_t) / float32(K)``, one float32 division (what ``np.mean`` of the
    reference's float32 array gives, the counts being exact); shut where ``u_t < float64(share_t)``.  No latch and no
    deviation: the reference has neither in this branch.

The column holds ``float32(gripper_close_cmd)`` where shut, else ``float32(gripper_open_cmd)``.

Departures from ``AutograspSampler``'s bits
    (a) Philox in place of the global NumPy stream, for the moves and for the uniforms.
    (b) The height is read from the float32 moves, not from the float64 ones.
    (c) The parent's bounded rejection loop applies: after ``max_trials`` rejected draws the last one is clipped
        (``n_capped``), where the reference would loop for ever.
"""
import numpy as np

from .autograsp_sampler import AutograspSampler
from .philox_gaussian_sampler import PhiloxGaussianCEMSampler, philox4x32_10, MAX_WIDTH

GRIP_TRIAL = 0xFFFFFFFE
LIFT = 2                    # the move channel the height follows
GRIP_HPARAMS = ('deviation_prob', 'reopen', 'action_norm_factor', 'z_thresh', 'gripper_close_cmd', 'gripper_open_cmd',
                'no_refit')


def grip_uniforms(key, call, samples, T):
    """``u [n, T]`` (float64) of sampling call ``call``: step ``t`` of sample ``i`` takes word ``t % 4`` of the counter
    ``(t // 4, 0xFFFFFFFE, i, call)``."""
    samples = np.asarray(samples, dtype=np.uint64).reshape(-1)
    blocks = (T + 3) // 4
    ctr = np.empty((samples.size, blocks, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(blocks, dtype=np.uint64)[None]
    ctr[..., 1] = np.uint64(GRIP_TRIAL)
    ctr[..., 2] = samples[:, None]
    ctr[..., 3] = np.uint64(call)
    words = philox4x32_10(ctr, key).astype(np.float64).reshape(samples.size, blocks * 4)[:, :T]
    return words / 4294967296.0


def commands(shut, hp):
    """Decisions -> the float32 column: ``float32(gripper_close_cmd)`` where shut, else ``float32(gripper_open_cmd)``."""
    return np.where(shut, np.float32(hp.gripper_close_cmd), np.float32(hp.gripper_open_cmd)).astype(np.float32)


def heights(moves32, state_z, hp):
    """``h [M, T]`` (float64) of the float32 moves ``[M, T, >= 3]``: the sequential sums of the module docstring."""
    m = np.asarray(moves32)
    if m.dtype != np.float32:
        raise TypeError('the height is a function of the float32 moves, got %s' % m.dtype)
    steps = m[:, :, LIFT].astype(np.float64) * float(hp.action_norm_factor)
    return np.cumsum(steps, axis=1) + float(state_z)        # (cumsum adds in order: c_0 = p_0, c_t = c_{t-1} + p_t)


def gripper_from_moves(moves32, state_z, hp, key, call, sample_indices, with_latched=False):
    """The gripper column ``[M, T]`` (float32) by height of the float32 moves ``moves32 [M, T, >= 3]`` of the samples
    ``sample_indices`` of sampling call ``call``.  ``with_latched``: also the decisions before and after the latch."""
    h = heights(moves32, state_z, hp)
    below = h < float(hp.z_thresh)
    shut = below.copy()
    if not hp.reopen:
        shut = np.logical_or.accumulate(shut, axis=1)
    latched = shut.copy()
    if hp.deviation_prob:
        u = grip_uniforms(key, call, sample_indices, h.shape[1])
        shut = np.logical_xor(shut, u < float(hp.deviation_prob))
    grip = commands(shut, hp)
    return (grip, below, latched) if with_latched else grip


def grip_margin(moves32, state_z, hp):
    """``min |h_t - z_thresh|`` over the samples and steps: how far the nearest height is from flipping its decision."""
    h = heights(moves32, state_z, hp)
    return float(np.nanmin(np.abs(h - float(hp.z_thresh)))) if h.size else np.inf


def elite_share(elite_plans, hp, column):
    """``share [T]`` (float32) of the elites ``[K, T, > column]`` that are shut at every step."""
    e = np.asarray(elite_plans)[:, :, column]
    count = (e == np.float32(hp.gripper_close_cmd)).sum(axis=0)
    return count.astype(np.float32) / np.float32(e.shape[0])


def gripper_from_share(share, hp, key, call, sample_indices):
    """The gripper column ``[M, T]`` (float32) by the elites' share ``share [T]`` (float32)."""
    share = np.asarray(share)
    u = grip_uniforms(key, call, sample_indices, share.shape[0])
    return commands(u < share.astype(np.float64)[None], hp)


class PhiloxAutograspSampler(PhiloxGaussianCEMSampler):
    def __init__(self, hp, adim, sdim, **kwargs):
        if adim - 1 < LIFT + 1:
            raise ValueError('PhiloxAutograspSampler needs at least 3 move channels (the height reads channel 2), got adim = %d'
                             % adim)
        n_tail = len(hp.get('append_action') or ())
        if adim + n_tail > MAX_WIDTH:
            raise ValueError('adim + len(append_action) = %d exceeds %d' % (adim + n_tail, MAX_WIDTH))
        if int(hp.max_trials) >= GRIP_TRIAL:
            raise ValueError('max_trials = %d reaches the trial word of the gripper uniforms (0x%X)' % (hp.max_trials, GRIP_TRIAL))
        if not 0.0 <= float(hp.deviation_prob) <= 1.0:
            raise ValueError('deviation_prob = %r outside [0, 1]' % (hp.deviation_prob,))
        super(PhiloxAutograspSampler, self).__init__(hp, adim - 1, sdim, **kwargs)
        self._state_z = 0.0
        self.last_grip_margin = np.inf  # least |height - z_thresh| of the last call by height (inf: by share)
        self.last_share = None          # the elites' share of the last call by share

    @staticmethod
    def get_default_hparams():
        params = PhiloxGaussianCEMSampler.get_default_hparams()
        theirs = AutograspSampler.get_default_hparams()
        params.update({name: theirs[name] for name in GRIP_HPARAMS})
        return params

    device_cem_driver = 'DeviceAutograspCEM'    # the class of device_cem.py that runs this sampler on the GPU

    def action_width(self):
        return self._adim + 1           # moves and gripper

    def start_planning_call(self, current_state):
        """The height the planning call starts from: ``current_state[2]``."""
        self._state_z = float(current_state[2])

    def state_z(self):
        return self._state_z

    def by_share(self, itr):
        """Does sampling call ``itr`` of a planning call (0: the first proposal) take the gripper from the elites' share?"""
        return itr > 0 and not self._hp.no_refit

    # ------------------------------------------------------------------ proposals
    def sample_initial_actions(self, t, nsamples, current_state):
        self.start_planning_call(current_state)
        self.initial_proposal(t)
        return self.sample_by_height(self.draws_for(nsamples))

    def sample_next_actions(self, n_samples, best_actions, scores):
        self.refit(best_actions)        # (the first adim - 1 columns: elite_rows)
        M = self.draws_for(n_samples)
        if self._hp.no_refit:
            return self.sample_by_height(M)
        return self.sample_by_share(M, best_actions)

    def sample_by_height(self, M):
        """``M`` draws of the current proposal ``[M, T, adim]``: float64 moves, the gripper by height of their float32 values."""
        moves = self._sample(M)
        call, moves32 = self._call - 1, moves.astype(np.float32)
        grip = gripper_from_moves(moves32, self._state_z, self._hp, self.key, call, np.arange(M))
        self.last_grip_margin, self.last_share = grip_margin(moves32, self._state_z, self._hp), None
        return np.concatenate((moves, grip[:, :, None].astype(np.float64)), axis=-1)

    def sample_by_share(self, M, elite_plans):
        """``M`` draws of the current proposal, the gripper by the share of ``elite_plans [K, T, >= adim]`` (column
        ``adim - 1``) that is shut."""
        moves = self._sample(M)
        self.last_share = elite_share(elite_plans, self._hp, self._adim)
        self.last_grip_margin = np.inf
        grip = gripper_from_share(self.last_share, self._hp, self.key, self._call - 1, np.arange(M))
        return np.concatenate((moves, grip[:, :, None].astype(np.float64)), axis=-1)
