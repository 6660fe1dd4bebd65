"""Cases and drivers shared by ``tools/make_golden_folding.py`` (which runs them on the reference's classes) and
``tests/test_folding_sampler.py`` (which runs them on this project's): one definition, so the two cannot drift apart.
Everything here is a pure function of its arguments and the global NumPy RNG; the caller passes the classes."""
import contextlib
import io
import warnings

import numpy as np

TOWEL_STD = dict(initial_std=0.005, initial_std_lift=0.05)      # experiments/sawyer/towel_classifier/hparams.py

# name, overrides of the sampler defaults, M, current state (xy is what the sampler keeps)
FOLDING_CASES = [
    ('towel_m18', dict(TOWEL_STD), 18, [0.9, 0.1, 0.2, 0., 0.]),
    ('towel_m36', dict(TOWEL_STD), 36, [0.2, 0.7, 0.1, 0.3, 1.]),
    ('towel_steps6', dict(TOWEL_STD, nactions=6), 18, [0.5, 0.5, 0.2, 0., 0.]),
    ('towel_split09', dict(TOWEL_STD, split_frac=0.9), 36, [0.05, 0.95, 0.2, 0., 0.]),
    ('defaults_repeat2', dict(repeat=2), 18, [0.3, 0.4, 0.2, 0., 0.]),
]
FOLDING_SEED0 = 300
N_ELITE = 10

# label -> (overrides, adim, M): what must raise, and where (constructor or first draw)
FOLDING_ERRORS = {
    'M200': (dict(TOWEL_STD), 4, 200),
    'nactions7': (dict(TOWEL_STD, nactions=7), 4, 18),
    'nactions4': (dict(TOWEL_STD, nactions=4), 4, 18),
    'adim5': (dict(TOWEL_STD), 5, 18),
}

# name, overrides, current state.  initial_std_lift 0.15 over 15 steps around a start height of 0.2 with z_thresh 0.15:
# some sequences cross the threshold and some do not (the tool asserts both occur)
# The reference's rejection sampling (the default) reads a ``stochastic_planning`` hyper-parameter that no class defines
# (``gaussian_sampler.py:140``), so the cases switch it off - or, once, set that attribute as ``tools/make_golden.py`` does.
PLAIN_DRAWS = dict(rejection_sampling=False)
AUTOGRASP_CASES = [
    ('stay_shut', dict(PLAIN_DRAWS), [0., 0., 0.2, 0., 0.]),
    ('reopen', dict(PLAIN_DRAWS, reopen=True), [0., 0., 0.2, 0., 0.]),
    ('deviate', dict(PLAIN_DRAWS, deviation_prob=0.3), [0., 0., 0.2, 0., 0.]),
    ('reopen_deviate', dict(PLAIN_DRAWS, reopen=True, deviation_prob=0.3, action_norm_factor=2.0, z_thresh=0.1),
     [0., 0., 0.25, 0., 0.]),
    ('refit_gripper', dict(PLAIN_DRAWS, no_refit=False), [0., 0., 0.2, 0., 0.]),
    ('refit_gripper_deviate', dict(PLAIN_DRAWS, no_refit=False, deviation_prob=0.3, gripper_close_cmd=2), [0., 0., 0.2, 0., 0.]),
    ('rejection', dict(stochastic_planning=None), [0., 0., 0.2, 0., 0.]),
]
AUTOGRASP_SEED0 = 400
AUTOGRASP_M = 24

TRACE_SEED = 500
TRACE_STEPS = 4             # replan_interval 2: planning calls at t = 0 and t = 2
TRACE_POLICY = dict(TOWEL_STD, num_samples=18, selection_frac=0.05, replan_interval=2, verbose=False)
TRACE_AGENT = {'adim': 4, 'sdim': 5}


@contextlib.contextmanager
def quiet():
    """No prints, and not NumPy's warning that a covariance refitted on fewer elites than dimensions is singular."""
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        yield


def hp_for(hparams_cls, sampler_cls, **over):
    hp = hparams_cls(replan_interval=0)
    for k, v in sampler_cls.get_default_hparams().items():
        hp.add_hparam(k, v)
    for k, v in over.items():
        setattr(hp, k, v)
    return hp


def fake_rollout_scores(actions):
    """Deterministic stand-in for ``evaluate_rollouts``: distance of the path's end from a target plus a rotation penalty."""
    a = np.asarray(actions, dtype=np.float64)
    end = np.cumsum(a[:, :, :3], axis=1)[:, -1]
    return np.sqrt(((end - np.array([0.6, -0.4, 0.5])) ** 2).sum(axis=-1)) + 0.05 * np.abs(a[:, :, 3]).sum(axis=1)


def run_folding_case(hparams_cls, sampler_cls, index):
    name, over, M, state = FOLDING_CASES[index]
    hp = hp_for(hparams_cls, sampler_cls, **over)
    with quiet():
        smp = sampler_cls(hp, 4, 5)
        np.random.seed(FOLDING_SEED0 + index)
        a0 = smp.sample_initial_actions(1, M, np.array(state))
        out = {'a0': a0, 'mean0': np.array(smp._base_mean), 'sigma0': np.array(smp._full_sigma)}
        scores = fake_rollout_scores(a0)
        best = scores.argsort()[:N_ELITE]
        out['a1'] = smp.sample_next_actions(M, a0[best].copy(), scores[best].copy())
        out['base_mean'], out['full_sigma'] = np.array(smp._base_mean), np.array(smp._full_sigma)
    return {name + '/' + k: v for k, v in out.items()}


def folding_error(hparams_cls, sampler_cls, label):
    """-> name of the exception type the constructor or the first draw raises (None: neither raises)."""
    over, adim, M = FOLDING_ERRORS[label]
    try:
        with quiet():
            smp = sampler_cls(hp_for(hparams_cls, sampler_cls, **over), adim, 5)
            np.random.seed(1)
            smp.sample_initial_actions(1, M, np.zeros(5))
    except Exception as e:      # noqa
        return type(e).__name__
    return None


def run_autograsp_case(hparams_cls, sampler_cls, index):
    """Initial draw, then a refit on its ten best -> arrays; a refit that raises is recorded by the caller."""
    name, over, state = AUTOGRASP_CASES[index]
    hp = hp_for(hparams_cls, sampler_cls, **over)
    with quiet():
        smp = sampler_cls(hp, 4, 5)
        np.random.seed(AUTOGRASP_SEED0 + index)
        a0 = smp.sample_initial_actions(1, AUTOGRASP_M, np.array(state))
        scores = fake_rollout_scores(a0)
        best = scores.argsort()[:N_ELITE]
        a1 = smp.sample_next_actions(AUTOGRASP_M, a0[best].copy(), scores[best].copy())
    return {name + '/a0': a0, name + '/a1': a1}


def autograsp_refit_error(hparams_cls, sampler_cls):
    """-> name of the exception type a refit of the class as it stands raises (None: it does not)."""
    hp = hp_for(hparams_cls, sampler_cls, **PLAIN_DRAWS)
    with quiet():
        smp = sampler_cls(hp, 4, 5)
        np.random.seed(2)
        a0 = smp.sample_initial_actions(1, AUTOGRASP_M, np.array([0., 0., 0.2, 0., 0.]))
        try:
            smp.sample_next_actions(AUTOGRASP_M, a0[:N_ELITE].copy(), np.arange(float(N_ELITE)))
        except Exception as e:      # noqa
            return type(e).__name__
    return None


def run_act_trace(controller_cls, sampler_cls):
    """``controller_cls`` (a ``CEMBaseController``) with the folding sampler and ``fake_rollout_scores`` as its cost,
    ``TRACE_STEPS`` control steps -> arrays (actions, elite indices and scores of every step) and the replan trace."""
    class Scored(controller_cls):
        def evaluate_rollouts(self, actions, cem_itr):
            return fake_rollout_scores(actions)

    arrays, trace = {}, []
    with quiet():
        ctrl = Scored(dict(TRACE_AGENT), dict(TRACE_POLICY, sampler=sampler_cls))
        ctrl.reset()
        np.random.seed(TRACE_SEED)
        states = np.random.RandomState(TRACE_SEED).uniform(0, 1, (TRACE_STEPS, 5))
        for t in range(TRACE_STEPS):
            out = ctrl.act(t=t, i_tr=0, state=states[:t + 1])
            arrays['trace/t%d/action' % t] = np.array(out['actions'])
            arrays['trace/t%d/best_indices' % t] = np.array(ctrl._best_indices)
            for k, v in out['plan_stat'].items():
                arrays['trace/t%d/%s' % (t, k)] = np.array(v)
            trace.append(ctrl._t_since_replan)
    return arrays, trace
