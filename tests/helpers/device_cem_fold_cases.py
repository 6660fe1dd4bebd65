"""``cem_sample_fold_kernel`` of ``csrc/vf_cem.h`` (with ``cem_refit_kernel`` as its refit) against its specification,
``PhiloxFoldingCEMSampler``, on synthetic scores.

Shared by ``tests/test_gpu_device_cem_folding.py`` (which asserts) and ``tools/device_cem_frames_bench.py`` (which records the
largest ulp distance seen).  Structured as ``device_cem_cases.py``; ``twin_run`` needs no GPU.
"""
import numpy as np

from tests.helpers.device_cem_cases import with_tail, ulp_distance                          # noqa: F401
from tests.helpers.device_cem_corr_cases import action_excess                               # noqa: F401
from visual_foresight_amd.hparams import HParams
from visual_foresight_amd.policy.cem_controllers.samplers.philox_folding_sampler import (
    PhiloxFoldingCEMSampler, select_elites)

TOWEL_STD = dict(initial_std=0.005, initial_std_lift=0.05)      # experiments/sawyer/towel_classifier/hparams.py
STATE = [0.9, 0.1, 0.2, 0., 0.]

# name -> (M, nactions, repeat, K, sampler hyper-parameters, append_action): the smallest shapes that reach each path
CASES = {
    'one_each': (3, 5, 3, 2, dict(TOWEL_STD, sampler_seed=41), None),           # one sample per family
    'towel': (18, 5, 3, 5, dict(TOWEL_STD, sampler_seed=42), None),
    'r_gt_d': (48, 5, 3, 24, dict(TOWEL_STD, sampler_seed=43), None),           # R = 24 > D = 20
    'past_script': (12, 7, 1, 4, dict(sampler_seed=44), None),                  # steps past the script
    'both_halves': (12, 20, 1, 4, dict(sampler_seed=45), None),                 # D = 80: both owned dimensions
    'all_blocks': (258, 5, 3, 256, dict(TOWEL_STD, sampler_seed=46), None),        # R = 256: all 64 Philox blocks
    'tail': (18, 5, 3, 5, dict(TOWEL_STD, sampler_seed=47), [0.25]),
}


def make_sampler(**over):
    hp = HParams(replan_interval=0)
    for k, v in PhiloxFoldingCEMSampler.get_default_hparams().items():
        hp.add_hparam(k, v)
    for k, v in over.items():
        if k in hp:
            setattr(hp, k, v)
        else:
            hp.add_hparam(k, v)
    return PhiloxFoldingCEMSampler(hp, 4, 5)


def case_scores(M, refit):
    """Synthetic scores of refit ``refit`` of a case: a tie inside and, from 6 samples on, a tie for the first place and one
    NaN - one only, so that K = M - 2 elites of the widest case are all numbers."""
    s = np.random.RandomState(300 + 10 * M + refit).normal(1.0, 0.5, M)
    s[1] = s[2] = np.sort(s)[1]
    if M >= 6:
        s[4] = np.nan
        s[0] = s[5] = np.nanmin(s) - 1.0
    return s


def twin_run(name, fed=None):
    """The specification's side of a case: the first proposal (call 0) and two refits on synthetic scores (calls 1, 2), every
    refit on the call before it - the twin's own candidates as float32, or the kernels' (``fed [2][M, T, W]``)."""
    M, nactions, repeat, K, over, tail = CASES[name]
    s = make_sampler(nactions=nactions, repeat=repeat, **over)
    out = {'sampler': s, 'tail': tail, 'K': K, 'M': M, 'calls': [], 'scores': [], 'elites': [], 'elite_plans': [], 'fit_mean': [],
           'fit_A': []}
    mean, std = s.initial_proposal(1, np.array(STATE))
    out['mean0'], out['std0'] = mean, std
    out['calls'].append(with_tail(s._sample(M), tail))
    for refit in range(2):
        scores = case_scores(M, refit)
        scored = np.asarray(out['calls'][-1].astype(np.float32) if fed is None else fed[refit], dtype=np.float64)
        elites = select_elites(scores, K)
        s.refit(scored[elites])
        out['scores'].append(scores)
        out['elites'].append(elites)
        out['elite_plans'].append(scored[elites])
        out['fit_mean'].append(s._mean.copy())
        out['fit_A'].append(s._A.copy())
        out['calls'].append(with_tail(s._sample(M), tail))
    return out


def device_run(name, device='cuda:0'):
    """The kernels' side of the same case -> (device results, the twin fed the kernels' scored candidates)."""
    import torch
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceFoldingCEM
    first = twin_run(name)
    s, K, M = first['sampler'], first['K'], first['M']
    dc = DeviceFoldingCEM(s, K, 3, M, device, first['tail'])      # (the sampler carries the case's start xy)
    dc.upload(first['mean0'], np.diag(first['std0']))
    got = {'elites': [], 'elite_scores': [], 'elite_plans': [], 'fit_mean': [], 'fit_A': [], 'R': []}
    dc.sample(0, M, 0)
    for refit in range(2):
        scores_dev = torch.from_numpy(first['scores'][refit]).to(dc.device)
        dc.refit(refit, scores_dev, dc.actions[refit])
        got['elite_plans'].append(dc.elite_plans.cpu().numpy())
        R, mean, A = dc.read_proposal()
        got['R'].append(R)
        got['fit_mean'].append(mean)
        got['fit_A'].append(A)
        dc.sample(refit + 1, M, refit + 1)
    torch.cuda.synchronize(dc.device)
    got['calls'] = [dc.actions[call].cpu().numpy() for call in range(3)]
    for refit in range(2):
        got['elites'].append(dc.elite_index[refit].cpu().numpy().astype(np.int64))
        got['elite_scores'].append(dc.elite_score[refit].cpu().numpy())
    want = twin_run(name, fed=got['calls'][:2])
    return got, want
