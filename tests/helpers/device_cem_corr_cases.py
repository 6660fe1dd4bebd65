"""The correlated-noise kernels of ``csrc/vf_cem.h`` against their specification, ``PhiloxCorrelatedNoiseSampler``, on
synthetic scores.

Shared by ``tests/test_gpu_device_cem_correlated.py`` (which asserts) and ``tools/device_cem_corr_bench.py`` (which records
how many values differ at all).  Structured as ``device_cem_cases.py``; ``twin_run`` needs no GPU.
"""
import contextlib
import io

import numpy as np

from tests.helpers.device_cem_cases import synthetic_scores, with_tail, ulp_distance      # noqa: F401
from visual_foresight_amd.hparams import HParams
from visual_foresight_amd.policy.cem_controllers.samplers.philox_correlated_sampler import (
    PhiloxCorrelatedNoiseSampler, select_elites)

STD = [0.05, 0.05, 0.2, np.pi / 10, 0.1, 0.3, 0.02, 1.0]

# name -> (M, K, nactions, adim, sampler hyper-parameters, append_action, logged last action, scores)
# The smallest shapes that reach each code path.  K = 100 elites need at least 100 scored candidates: ``cov_wide`` scores the
# candidates of TWO sampling calls of M = 64, as ``r_gt_d`` of the Gaussian cases does.
CASES = {
    'franka': (200, 20, 10, 4, dict(sampler_seed=31), None, None, 'normal'),
    'two_halves': (7, 3, 15, 5, dict(sampler_seed=32), None, None, 'normal'),
    'full': (4, 2, 16, 8, dict(sampler_seed=33), None, None, 'normal'),
    'one_step': (2, 2, 1, 1, dict(sampler_seed=34), None, None, 'normal'),
    'cov': (40, 20, 10, 4, dict(sampler_seed=35, refit_cov=True), None, None, 'normal'),
    'cov_wide': (64, 100, 15, 5, dict(sampler_seed=36, refit_cov=True), None, None, 'normal'),
    'smooth_tail': (33, 6, 4, 4, dict(sampler_seed=37, smooth_across_last_action=True, mean_bias=[0.01, -0.02, 0.0, 0.3],
                                      kappa=3, beta_0=0.7, beta_1=0.3),
                    [0.25, -1.0], [0.03, -0.01, 0.2, -0.4, 0.25, -1.0], 'normal'),
    'ties': (40, 10, 5, 4, dict(sampler_seed=38), None, None, 'ties_nan'),
}


def make_sampler(adim, **over):
    hp = HParams(replan_interval=0)
    for k, v in PhiloxCorrelatedNoiseSampler.get_default_hparams().items():
        hp.add_hparam(k, v)
    over.setdefault('initial_std', STD[:adim])
    for k, v in over.items():
        if k in hp:
            setattr(hp, k, v)
        else:
            hp.add_hparam(k, v)
    return PhiloxCorrelatedNoiseSampler(hp, adim, 5)


def f64_ulp_distance(a, b):
    """Distance in float64 units of least precision between two finite float64 arrays of one sign pattern."""
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)


def centre_bound(flat, soft):
    """The issue's bound on ``|centre_d - twin|``: ``(K + 4) * 2**-51 * sum_k |e_kd| soft_k / den``."""
    K = flat.shape[0]
    den = float(np.sum(soft)) + 1e-4
    return (K + 4) * 2.0 ** -51 * (np.abs(flat) * soft[:, None]).sum(axis=0) / den


def action_excess(device, twin):
    """Per value of one sampling call: how far the device's float32 action is outside the tolerance
    ``max(1 float32 ulp, 2**-40 * max|twin actions of that call|)`` (<= 0: inside) and its ulp distance."""
    twin32 = np.asarray(twin).astype(np.float32)
    ulps = ulp_distance(device, twin32)
    floor = 2.0 ** -40 * float(np.abs(twin).max())
    delta = np.abs(np.asarray(device, np.float64) - twin32.astype(np.float64))
    return np.where(ulps <= 1, 0.0, delta - floor), ulps


def twin_run(name, scored_candidates=None):
    """The specification's side of a case.  Sampling calls 0 and 1 draw the first proposal, the scored candidates - call 0's,
    or both calls' when K > M; the caller's float32 ones when given, which is how the kernels' own candidates are fed back -
    are refitted on synthetic scores, call 2 draws from the fit."""
    M, K, nactions, adim, over, tail, logged, kind = CASES[name]
    s = make_sampler(adim, nactions=nactions, **over)
    if logged is not None:
        s.log_best_action(np.asarray(logged, np.float64), None)
    out = {'sampler': s, 'tail': tail, 'K': K, 'M': M, 'adim': adim}
    calls = []
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(2):
            s.start_planning_call()
            calls.append(with_tail(s._sample(M), tail))
        n_scored = 2 * M if K > M else M
        out['n_scored'] = n_scored
        scores = synthetic_scores(kind, n_scored, 100 + M)
        if scored_candidates is None:
            scored_candidates = np.concatenate(calls)[:n_scored].astype(np.float32)
        scored = np.asarray(scored_candidates, dtype=np.float64)
        elites = select_elites(scores, K)
        s.refit(scored[elites][:, :, :adim], scores[elites])
        calls.append(with_tail(s._sample(M), tail))
    out.update(scores=scores, elites=elites, elite_plans=scored[elites], soft=s.last_soft.copy(), centre=s.last_centre.copy(),
               elite_rows=scored[elites][:, :, :adim].reshape(K, -1), calls=calls)
    if s._hp.refit_cov:
        out.update(fit_mean=s.last_mean.copy(), fit_A=s._A.copy())
    return out


def device_run(name, device='cuda:0'):
    """The kernels' side of the same case -> (device results, the twin fed the kernels' scored candidates)."""
    import torch
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceCorrelatedCEM
    first = twin_run(name)
    s, K, M, n_scored = first['sampler'], first['K'], first['M'], first['n_scored']
    dc = DeviceCorrelatedCEM(s, K, 3, M, device, first['tail'])
    dc.upload()
    for call in range(2):
        dc.sample(call, M, call)
    scored = dc.actions[:2].reshape(2 * M, dc.T, dc.W)[:n_scored]
    scores_dev = torch.from_numpy(first['scores']).to(dc.device)
    dc.refit(0, scores_dev, scored)
    dc.sample(2, M, 2)
    torch.cuda.synchronize(dc.device)
    got = {'calls': [dc.actions[call].cpu().numpy() for call in range(3)]}
    got['elites'] = dc.elite_index[0].cpu().numpy().astype(np.int64)
    got['elite_scores'] = dc.elite_score[0].cpu().numpy()
    got['elite_plans'] = dc.elite_plans.cpu().numpy()
    got.update(dc.read_proposal(), scored=scored.cpu().numpy())
    want = twin_run(name, scored_candidates=got['scored'])
    return got, want
