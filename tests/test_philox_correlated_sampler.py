"""``PhiloxCorrelatedNoiseSampler`` on the CPU: pinned to ``CorrelatedNoiseSampler`` (which is pinned to the reference) by
feeding that class this sampler's normals, the refit against the reference class's, refusals, the call counter, determinism,
the library's new exports and the controller's host route."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from tests.helpers.fake_predictor import make_fake_predictor_class
from visual_foresight_amd.hparams import HParams
from visual_foresight_amd.policy.cem_controllers import PixelCostController
from visual_foresight_amd.policy.cem_controllers.samplers import CorrelatedNoiseSampler, PhiloxCorrelatedNoiseSampler
from visual_foresight_amd.policy.cem_controllers.samplers import philox_correlated_sampler as pcs
from visual_foresight_amd.policy.cem_controllers.samplers import philox_gaussian_sampler as pgs


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def hp_for(cls=PhiloxCorrelatedNoiseSampler, **over):
    hp = HParams(replan_interval=0)
    for k, v in cls.get_default_hparams().items():
        hp.add_hparam(k, v)
    for k, v in over.items():
        if k in hp:
            setattr(hp, k, v)
        else:
            hp.add_hparam(k, v)
    return hp


def make(**over):
    over.setdefault('sampler_seed', 1234)
    return PhiloxCorrelatedNoiseSampler(hp_for(**over), 4, 5)


def reference_for(sampler):
    """The reference-pinned class under the same hyper-parameters."""
    return CorrelatedNoiseSampler(sampler._hp, 4, 5)


@contextlib.contextmanager
def philox_for_np_random(sampler, call):
    """``np.random.normal(size=(n, nactions, adim))`` returns the sampler's white normals of sampling call ``call``."""
    original = np.random.normal

    def normal(size):
        n, nactions, adim = size
        return pgs.standard_normals(sampler.key, call, np.arange(n), 0, nactions * adim).reshape(size)
    np.random.normal = normal
    try:
        yield
    finally:
        np.random.normal = original


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ----------------------------------------------------------------------------- pinned to the reference-pinned class
@pytest.mark.parametrize('over,logged', [
    ({}, False),
    ({'mean_bias': [0.01, -0.02, 0.0, 0.3]}, False),
    ({'smooth_across_last_action': True}, True),
    ({'smooth_across_last_action': True, 'mean_bias': [0.01, -0.02, 0.0, 0.3]}, False),
    ({'nactions': 1}, False),
    ({'nactions': 1, 'smooth_across_last_action': True}, True),
    ({'nactions': 10, 'beta_0': 0.7, 'beta_1': 0.3, 'initial_std': [0.1, 0.03, 0.2]}, False),
])
def test_first_proposal_is_the_reference_filter_bit_for_bit(over, logged):
    """``CorrelatedNoiseSampler._sample_noise`` fed this sampler's normals equals the first proposal: the operations and
    their order are the same."""
    s = make(**over)
    ref = reference_for(s)
    if logged:
        action = np.array([0.03, -0.01, 0.2, -0.4])[:s._adim]
        s.log_best_action(action, None)
        ref.log_best_action(action, None)
    with quiet():
        for call in range(2):
            got = s.sample_initial_actions(0, 9, None)
            with philox_for_np_random(s, call):
                want = ref.sample_initial_actions(0, 9, None)
            assert got.shape == want.shape == (9, s._hp.nactions, s._adim)
            np.testing.assert_array_equal(bits(got), bits(want))
    if s._hp.nactions == 1 and not logged:      # the wrap-around predecessor is the step itself, unfiltered
        w = pgs.standard_normals(s.key, 1, np.arange(9), 0, s._D)
        shaped = w * np.asarray(s._hp.initial_std)[None]
        np.testing.assert_array_equal(got[:, 0], 0.5 * shaped + 0.5 * shaped)


@pytest.mark.parametrize('refit_cov', [False, True])
@pytest.mark.parametrize('kappa,K', [(1, 10), (3, 4), (1, 30)])
def test_sample_next_actions_is_the_reference_refit(refit_cov, kappa, K):
    """Without ``refit_cov`` only ``np.sum``'s order differs (rtol 1e-12); with it ``(w A) A^T`` stands against
    ``w @ np.cov`` (rtol 1e-9, atol 1e-15)."""
    s = make(refit_cov=refit_cov, kappa=kappa, nactions=5)
    ref = reference_for(s)
    rs = np.random.RandomState(K)
    elites = rs.normal(0, 0.1, (K, 5, 4))
    scores = np.sort(rs.normal(1.0, 0.5, K))
    with quiet():
        s.sample_initial_actions(0, 3, None)            # (call 0)
        got = s.sample_next_actions(12, elites, scores)
        with philox_for_np_random(s, 1):
            want = ref.sample_next_actions(12, elites, scores)
    assert got.shape == (12, 5, 4)
    if refit_cov:
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(s._A @ s._A.T, np.cov(elites.reshape(K, -1), rowvar=False), rtol=0, atol=1e-15)
        assert s._A.shape == (20, K)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    soft = np.exp(kappa * (scores[0] - scores))
    np.testing.assert_array_equal(s.last_soft, soft)
    np.testing.assert_allclose(s.last_centre, (elites * soft[:, None, None]).sum(0).reshape(-1) / (soft.sum() + 1e-4),
                               rtol=1e-13)


def test_first_proposal_adds_nothing_and_later_ones_add_the_centre():
    s = make(nactions=3)
    with quiet():
        a = s.sample_initial_actions(0, 6, None)
        b = s.sample_next_actions(6, a[:2], np.array([0.0, 1.0]))
        noise = s.ar1(s.shape(pgs.standard_normals(s.key, 1, np.arange(6), 0, 12)).reshape(6, 3, 4))
        np.testing.assert_array_equal(b, noise + s.last_centre.reshape(1, 3, 4))
        # a planning call starts without the previous one's centre
        c = s.sample_initial_actions(1, 6, None)
        np.testing.assert_array_equal(c, s.ar1(s.shape(pgs.standard_normals(s.key, 2, np.arange(6), 0, 12)).reshape(6, 3, 4)))


# ----------------------------------------------------------------------------- refusals, counter, determinism
def test_limits_are_refused():
    with pytest.raises(ValueError):
        make(nactions=33)                       # D = 132
    with pytest.raises(ValueError):
        make(initial_std=[0.1] * 5, append_action=[0.0] * 4)
    with pytest.raises(ValueError):
        make(num_samples=5000)
    make(nactions=32, num_samples=4096, append_action=[0.0] * 4)


def test_call_advances_once_per_sampling_call():
    s = make()
    assert s._call == 0
    with quiet():
        a = s.sample_initial_actions(0, 4, None)
        assert s._call == 1
        s.sample_next_actions(4, a[:2], np.zeros(2))
        assert s._call == 2
        s.sample_initial_actions(1, 4, None)
    assert s._call == 3 and s.next_call() == 3 and s._call == 4


def test_determinism_under_sampler_seed_and_np_random_seed():
    def run(**over):
        s = PhiloxCorrelatedNoiseSampler(hp_for(**over), 4, 5)
        with quiet():
            a = s.sample_initial_actions(0, 30, None)
            b = s.sample_next_actions(30, a[:10], np.arange(10.0))
        return s.key, a, b
    k1, a1, b1 = run(sampler_seed=(7 << 32) | 9)
    k2, a2, b2 = run(sampler_seed=(7 << 32) | 9)
    assert k1 == k2 == (9, 7)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    _, a3, _ = run(sampler_seed=10)
    assert not np.array_equal(a1, a3)
    np.random.seed(3)
    k4, a4, _ = run()
    np.random.seed(3)
    k5, a5, _ = run()
    np.random.seed(4)
    k6, a6, _ = run()
    assert k4 == k5 != k6
    np.testing.assert_array_equal(a4, a5)
    assert not np.array_equal(a4, a6)


# ----------------------------------------------------------------------------- the library (no GPU)
def test_library_exports_the_correlated_entry_points():
    from visual_foresight_amd import _lib
    from visual_foresight_amd.policy.cem_controllers.device_cem import corr_config, corr_workspace_bytes
    _lib.build_library()
    lib = _lib.load_library()
    for name in ('vf_cem_corr_workspace_bytes', 'vf_cem_soft_refit', 'vf_cem_sample_corr'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.vf_abi_version() == 7
    for over, K, tail in (({}, 10, None), ({'refit_cov': True}, 10, None), ({'refit_cov': True, 'nactions': 32}, 256, [1.0]),
                          ({'nactions': 1, 'initial_std': [0.1]}, 1, None)):
        s = make(**over)
        cfg = corr_config(s, K, tail)
        D = s._D
        want = 16 + 8 * (2 * D + K + (K * D if s._hp.refit_cov else 0))
        assert corr_workspace_bytes(D, K, s._hp.refit_cov) == want
        assert lib.vf_cem_corr_workspace_bytes(ctypes.byref(cfg)) == want
    s = make(mean_bias=[0.1, 0.2, 0.3, 0.4], kappa=3, beta_0=0.7, beta_1=0.3, smooth_across_last_action=True)
    s.log_best_action(np.array([1.0, 2.0, 3.0, 4.0, 9.0]), None)
    cfg = corr_config(s, 10, [9.0])
    assert (cfg.seed_lo, cfg.seed_hi, cfg.nactions, cfg.adim, cfg.tail, cfg.has_first_prev) == (1234, 0, 15, 4, 1, 1)
    assert (cfg.kappa, cfg.beta_0, cfg.beta_1) == (3.0, 0.7, 0.3)
    assert list(cfg.std)[:4] == [0.05, 0.05, 0.2, np.pi / 10] and list(cfg.bias)[:4] == [0.1, 0.2, 0.3, 0.4]
    assert list(cfg.first_prev)[:5] == [1.0, 2.0, 3.0, 4.0, 0.0] and cfg.tail_value[0] == 9.0

    def bad(message, **fields):
        c = corr_config(make(), 10)
        for k, v in fields.items():
            setattr(c, k, v)
        assert lib.vf_cem_corr_workspace_bytes(ctypes.byref(c)) == 0
        assert message in lib.vf_last_error(), lib.vf_last_error()
    bad(b'nactions', nactions=0)
    bad(b'adim', adim=0)
    bad(b'tail', tail=-1)
    bad(b'adim + tail', tail=5)
    bad(b'exceeds 128', nactions=33)
    bad(b'n_elites', n_elites=0)
    bad(b'n_elites', n_elites=257)
    bad(b'n_elites', n_elites=1, refit_cov=1)       # one elite has no covariance
    assert lib.vf_cem_corr_workspace_bytes(None) == 0 and b'null' in lib.vf_last_error()
    # refusals need no device: nothing is launched
    good = corr_config(make(), 10)
    assert lib.vf_cem_sample_corr(0, ctypes.byref(good), None, 0, 4, None, None) == -1
    assert b'null' in lib.vf_last_error()
    assert lib.vf_cem_sample_corr(0, ctypes.byref(good), 32, 0, 5000, 64, None) == -1 and b'M = 5000' in lib.vf_last_error()
    assert lib.vf_cem_sample_corr(0, ctypes.byref(good), 8, 0, 4, 64, None) == -1 and b'aligned' in lib.vf_last_error()
    assert lib.vf_cem_soft_refit(0, ctypes.byref(good), None, None, 20, None, None, None, None, None) == -1
    assert b'null' in lib.vf_last_error()
    assert lib.vf_cem_soft_refit(0, ctypes.byref(good), 64, 64, 9, 64, 64, 64, 64, None) == -1 and b'M = 9' in lib.vf_last_error()
    assert lib.vf_cem_soft_refit(-1, ctypes.byref(good), 64, 64, 20, 64, 64, 64, 64, None) == -1
    assert b'negative' in lib.vf_last_error()


# ----------------------------------------------------------------------------- the controller's host route
def test_controller_without_score_device_plans_on_the_host():
    T, H, W = 5, 16, 16
    fake = make_fake_predictor_class(T, H, W)
    assert not hasattr(fake, 'score_device')
    pol = dict(predictor_class=fake, verbose=False, sampler=PhiloxCorrelatedNoiseSampler, nactions=T, num_samples=40,
               sampler_seed=11, initial_std=[0.05, 0.05, 0.2, 0.3])
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    rs = np.random.RandomState(1)
    images, states = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8), rs.normal(0, 0.1, (2, 5))

    def plan():
        with quiet():
            ctrl = PixelCostController(ag, dict(pol), 0, 1)
            ctrl.reset()
            out = ctrl.act(t=1, i_tr=0, desig_pix=[[8, 8]], goal_pix=[[3, 12]], images=images, state=states)
        return ctrl, out
    ctrl, out = plan()
    assert isinstance(ctrl._sampler, PhiloxCorrelatedNoiseSampler) and ctrl._hp.device_cem is True
    assert ctrl._device_cem_plan() is None
    assert out['actions'].shape == (4,) and sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
    scores = out['plan_stat']['scores_itr2']
    np.testing.assert_array_equal(ctrl._best_indices, pgs.select_elites(scores, 10))
    np.testing.assert_array_equal(out['actions'], ctrl._best_actions[0, 0])
    assert np.sort(scores)[:10].mean() < np.sort(out['plan_stat']['scores_itr0'])[:10].mean()
    _, again = plan()
    np.testing.assert_array_equal(out['actions'], again['actions'])
    assert ctrl._sampler._call == 3 and ctrl._sampler.last_soft.shape == (10,) and ctrl._sampler.last_soft[0] == 1.0
    assert pcs.PhiloxCorrelatedNoiseSampler.device_cem_driver == 'DeviceCorrelatedCEM'
