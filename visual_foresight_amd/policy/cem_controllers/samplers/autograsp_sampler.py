"""Gaussian CEM proposal whose gripper channel follows the height (reference ``samplers/autograsp_sampler.py:5-58``).

The first ``adim - 1`` channels are a ``GaussianCEMSampler``'s.  The last one is not sampled but derived per sequence, the
way an auto-grasping environment would act: the gripper is commanded shut (``gripper_close_cmd``) at every step at which
the planned height - ``current_state[2]`` plus the cumulative z action times ``action_norm_factor`` - is below ``z_thresh``,
and open (``gripper_open_cmd``) elsewhere.  Unless ``reopen`` is set it stays shut from the first such step on.  With
``deviation_prob`` > 0 every step's command is flipped with that probability (one ``np.random.uniform`` draw of the
horizon's length per sequence, after the Gaussian draws; no draw at all when the probability is 0).

Refits: ``no_refit`` True (the default) derives the gripper of the refitted Gaussian's samples as above; False draws it
per time step from the share of elites that were shut at that step (one ``np.random.uniform(size=n_samples)`` per step).

One departure from the reference: its ``sample_next_actions`` calls the parent without ``scores`` and so raises
``TypeError`` on every refit (the class is usable there with ``iterations`` 1 only; ``tests/golden/folding_sampler.json``
records that).  Here ``scores`` is forwarded and refits work; the refitted draws are pinned against the reference's code
run with that one argument made optional.
"""
import numpy as np

from .gaussian_sampler import GaussianCEMSampler


class AutograspSampler(GaussianCEMSampler):
    def __init__(self, hp, adim, sdim, **kwargs):
        super(AutograspSampler, self).__init__(hp, adim - 1, sdim, **kwargs)
        self._current_state = None

    @staticmethod
    def get_default_hparams():
        params = GaussianCEMSampler.get_default_hparams()
        params.update({
            'deviation_prob': 0,            # chance of flipping a step's gripper command
            'reopen': False,                # may the gripper open again once it has shut
            'action_norm_factor': 1.0,      # z action -> height
            'z_thresh': 0.15,               # shut below this height
            'gripper_close_cmd': 1,
            'gripper_open_cmd': -1,
            'no_refit': True,               # refits derive the gripper from the height, too
        })
        return params

    def sample_initial_actions(self, t, nsamples, current_state):
        self._current_state = current_state
        moves = super(AutograspSampler, self).sample_initial_actions(t, nsamples, current_state)
        return self._sample_gripper(moves, nsamples)

    def sample_next_actions(self, n_samples, best_actions, scores):
        hp = self._hp
        moves = super(AutograspSampler, self).sample_next_actions(n_samples, best_actions[:, :, :-1], scores)
        if hp.no_refit:
            return self._sample_gripper(moves, n_samples)
        horizon = moves.shape[1]
        shut_share = np.mean((best_actions[:, :, -1] == hp.gripper_close_cmd).astype(np.float32), axis=0)
        grip = np.zeros((n_samples, horizon, 1), dtype=np.float32)
        for t in range(horizon):
            shut = np.random.uniform(size=n_samples) < shut_share[t]
            grip[:, t, 0] = shut * hp.gripper_close_cmd + np.logical_not(shut) * hp.gripper_open_cmd
        return np.concatenate((moves, grip), axis=-1)

    def _sample_gripper(self, moves, nsamples):
        hp = self._hp
        horizon = moves.shape[1]
        grip = np.zeros((nsamples, horizon, 1))
        for b in range(nsamples):
            height = np.cumsum(moves[b, :, 2] * hp.action_norm_factor) + self._current_state[2]
            shut = height < hp.z_thresh
            if not hp.reopen and shut.any():
                shut[np.argmax(shut):] = True
            if hp.deviation_prob:
                flip = np.random.uniform(size=horizon) < hp.deviation_prob
                shut = np.logical_xor(shut, flip)
            grip[b, :, 0] = np.logical_not(shut) * hp.gripper_open_cmd + shut * hp.gripper_close_cmd
        return np.concatenate((moves, grip), axis=-1)
