"""Device-resident CEM for the folding sampler: ``cem_sample_fold_kernel`` (and ``cem_refit_kernel`` as its refit) of
``csrc/vf_cem.h`` against ``PhiloxFoldingCEMSampler``.  No predictor: a first proposal and two refits on synthetic scores."""
import ctypes

import numpy as np
import pytest

from tests.helpers import device_cem_fold_cases as cases


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_kernels_match_the_twin(name):
    """Elite indices, scores and plans, ``mean`` and ``A`` bit for bit (the refit is ``vf_cem_refit``); actions within
    ``max(1 float32 ulp, 2^-40 max|twin actions of the call|)`` - the device's log / sin / cos are the only steps not correctly
    rounded, and a carry plus noise can cancel to near zero; the clip is continuous, so it needs no margin; the tail columns
    exact.  One MI355X (profiles/device_cem_frames.txt): no action value of any case differed from the twin at all."""
    got, want = cases.device_run(name)
    K = want['K']
    for refit in range(2):
        np.testing.assert_array_equal(got['elites'][refit], want['elites'][refit])
        np.testing.assert_array_equal(got['elite_scores'][refit], want['scores'][refit][want['elites'][refit]])
        np.testing.assert_array_equal(got['elite_plans'][refit], want['elite_plans'][refit].astype(np.float32))
        assert got['R'][refit] == K
        np.testing.assert_array_equal(got['fit_mean'][refit], want['fit_mean'][refit])
        np.testing.assert_array_equal(got['fit_A'][refit], want['fit_A'][refit])
    worst, worst_ulps, differing, total = [], 0, 0, 0
    for call, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        assert g.shape == w.shape and g.dtype == np.float32 and np.isfinite(g).all()
        excess, ulps = cases.action_excess(g[:, :, :4], w[:, :, :4])
        worst.append(float(excess.max()))
        worst_ulps = max(worst_ulps, int(ulps.max()))
        differing += int((ulps > 0).sum())
        total += ulps.size
        np.testing.assert_array_equal(g[:, :, 4:], w[:, :, 4:].astype(np.float32), err_msg='tail, call %d' % call)
    print('%s: %d of %d action values differ from the twin at all; largest distance %d float32 ulp'
          % (name, differing, total, worst_ulps))
    assert max(worst) <= 0.0, worst


@pytest.mark.gpu
def test_refusals_launch_nothing():
    import torch
    from visual_foresight_amd import _lib
    from visual_foresight_amd.policy.cem_controllers.device_cem import DeviceFoldingCEM, fold_config
    s = cases.twin_run('one_each')['sampler']
    dc = DeviceFoldingCEM(s, 2, 1, 18, 'cuda:0')
    dc.actions.fill_(7.0)
    lib = _lib.load_library()

    def launch(cfg, M, workspace=None):
        return lib.vf_cem_sample_fold(0, ctypes.byref(cfg), dc.workspace.data_ptr() if workspace is None else workspace, 0, M,
                                      dc.actions.data_ptr(), None)
    for change, M in ((dict(nactions=4), 18), (dict(nactions=33), 18), (dict(repeat=0), 18), (dict(tail=5), 18),
                      (dict(n_elites=1), 18), (dict(n_scripted=0), 18), (dict(n_scripted=10), 18), ({}, 0), ({}, 4097)):
        cfg = fold_config(s, 2, 18)
        for k, v in change.items():
            setattr(cfg, k, v)
        assert launch(cfg, M) != 0, (change, M)
        assert b'vf_cem_sample_fold' in lib.vf_last_error()
    assert launch(fold_config(s, 2, 18), 18, workspace=dc.workspace.data_ptr() + 8) != 0       # misaligned
    torch.cuda.synchronize()
    assert (dc.actions == 7.0).all()
