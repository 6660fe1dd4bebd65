"""The kernels of ``csrc/vf_cem.h`` against their specification, ``PhiloxGaussianCEMSampler``, on synthetic scores.

Shared by ``tests/test_gpu_device_cem.py`` (which asserts) and ``tools/device_cem_bench.py`` (which records how many values
differ at all).  ``twin_run`` needs no GPU: the seeds are checked there (no tested value within 1e-9 of a rejection limit or
of an integer that the discretisation floors at).
"""
import contextlib
import io

import numpy as np

from visual_foresight_amd.hparams import HParams
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import (
    PhiloxGaussianCEMSampler, select_elites)

# name -> (M, K, nactions, repeat, adim, sampler hyper-parameters, append_action, mean offset per column, scores)
# The first three are the issue's.  K = 100 elites need at least 100 scored candidates: that case scores the candidates of TWO
# sampling calls of M = 64 (128), which keeps M and K as stated and gives R = 100 > D = 75.  Its 45 limited values per
# sequence are all inside 1.5 std about once in 640 draws, so it runs with max_trials 8 (the float64 twin would otherwise
# take a minute): most of its samples are the clipped last draw, the accepted rest covers the other branch.
CASES = {
    'r_lt_d': (7, 3, 2, 1, 4, dict(sampler_seed=11), None, None, 'normal'),
    'default': (200, 10, 5, 3, 4, dict(sampler_seed=12), None, None, 'normal'),
    'r_gt_d': (64, 100, 15, 1, 5, dict(sampler_seed=13, max_trials=8), None, None, 'normal'),
    'ties_nan': (40, 10, 5, 3, 4, dict(sampler_seed=14), None, None, 'ties_nan'),
    'near_limit': (48, 10, 5, 3, 4, dict(sampler_seed=15), None, [0.03, -0.03, 0.05, 0.0], 'normal'),
    'capped': (12, 4, 3, 2, 4, dict(sampler_seed=16, max_trials=4), None, [1.0, 1.0, 1.0, 1.0], 'normal'),
    'no_rejection': (33, 6, 4, 2, 5, dict(sampler_seed=17, rejection_sampling=False, discrete_ind=[4], add_zero_action=True),
                     [0.25, -1.0], [0.08, 0.0, 0.0, 0.7, 2.0], 'normal'),
}


def make_sampler(adim, **over):
    hp = HParams(replan_interval=0)
    for k, v in PhiloxGaussianCEMSampler.get_default_hparams().items():
        hp.add_hparam(k, v)
    for k, v in over.items():
        if k in hp:
            setattr(hp, k, v)
        else:
            hp.add_hparam(k, v)
    return PhiloxGaussianCEMSampler(hp, adim, 5)


def synthetic_scores(kind, n, seed):
    s = np.random.RandomState(seed).normal(1.0, 0.5, n)
    if kind == 'ties_nan':
        s[3] = s[17] = s[5]             # a tie inside the elites ...
        s[8] = s[30] = np.nan           # ... NaN, which sorts last ...
        s[11], s[12] = 0.0, -0.0        # ... and the two zeros, equal
        s[20] = s[21] = s.min() - 1.0   # a tie for the first place
        s[np.argsort(s)[9]] = s[np.argsort(s)[10]]      # a tie across the K-th place
    return s


def with_tail(actions, tail):
    if not tail:
        return actions
    t = np.broadcast_to(np.asarray(tail, np.float64), actions.shape[:2] + (len(tail),))
    return np.concatenate((actions, t), axis=-1)


def ulp_distance(a, b):
    """Distance in float32 units of least precision between two float32 arrays (NaN against NaN is 0)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def twin_run(name, scored_candidates=None):
    """The specification's side of a case.  Sampling calls 0 and 1 draw from the initial proposal (its mean moved by the
    case's offset), the scored candidates - call 0's, or both calls' when K > M; the caller's float32 ones when given, which
    is how the kernels' own candidates are fed back - are refitted on synthetic scores, call 2 draws from the fit.
    -> dict of everything the kernels must reproduce, and ``margin``."""
    M, K, nactions, repeat, adim, over, tail, offset, kind = CASES[name]
    s = make_sampler(adim, nactions=nactions, repeat=repeat, **over)
    out = {'sampler': s, 'tail': tail, 'K': K, 'M': M}
    with contextlib.redirect_stdout(io.StringIO()):
        mean, std = s.initial_proposal(0)
    if offset is not None:
        s._mean = mean = mean + np.tile(np.asarray(offset, np.float64), nactions)
    out['mean0'], out['std0'] = mean, std
    margin = np.inf
    calls = []
    for _ in range(2):
        a = with_tail(s._sample(M), tail)
        calls.append(dict(actions=a, trials=s.last_trials.copy(), capped=s.last_capped.copy()))
        margin = min(margin, s.last_margin)
    n_scored = 2 * M if K > M else M
    out['n_scored'] = n_scored
    scores = synthetic_scores(kind, n_scored, 100 + M)
    if scored_candidates is None:
        scored_candidates = np.concatenate([c['actions'] for c in calls])[:n_scored].astype(np.float32)
    scored = np.asarray(scored_candidates, dtype=np.float64)
    elites = select_elites(scores, K)
    s.refit(scored[elites])
    out.update(scores=scores, elites=elites, elite_plans=scored[elites], fit_mean=s._mean.copy(), fit_A=s._A.copy())
    a = with_tail(s._sample(M), tail)
    calls.append(dict(actions=a, trials=s.last_trials.copy(), capped=s.last_capped.copy()))
    out['calls'] = calls
    out['margin'] = min(margin, s.last_margin)
    out['n_capped'] = s.n_capped
    return out


def device_run(name, device='cuda:0'):
    """The kernels' side of the same case -> (device results, the twin fed the kernels' scored candidates)."""
    import torch
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceCEM
    first = twin_run(name)
    s, K, M, n_scored = first['sampler'], first['K'], first['M'], first['n_scored']
    dc = DeviceCEM(s, K, 3, M, device, first['tail'])
    dc.upload(first['mean0'], np.diag(first['std0']))
    got = {'calls': []}
    for call in range(2):
        dc.sample(call, M, call)
    scored = dc.actions[:2].reshape(2 * M, dc.T, dc.W)[:n_scored]
    scores_dev = torch.from_numpy(first['scores']).to(dc.device)
    dc.refit(0, scores_dev, scored)
    dc.sample(2, M, 2)
    torch.cuda.synchronize(dc.device)
    for call in range(3):
        got['calls'].append(dict(actions=dc.actions[call].cpu().numpy(), trials=dc.trials[call].cpu().numpy(),
                                 capped=dc.capped[call].cpu().numpy() != 0))
    got['elites'] = dc.elite_index[0].cpu().numpy().astype(np.int64)
    got['elite_scores'] = dc.elite_score[0].cpu().numpy()
    got['elite_plans'] = dc.elite_plans.cpu().numpy()
    R, mean, A = dc.read_proposal()
    got.update(R=R, fit_mean=mean, fit_A=A, scored=scored.cpu().numpy())
    want = twin_run(name, scored_candidates=got['scored'])
    return got, want
