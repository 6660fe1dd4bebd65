"""``PhiloxAutograspSampler`` on the CPU: the moves against its parent, the gripper column against ``AutograspSampler``'s own
code, the elites' share, the uniform words, the refusals, one planning call on the host route, the library's entry, and the
seeds of the GPU cases."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests.helpers import device_cem_autograsp_cases as cases
from tests.helpers.fake_predictor import make_fake_predictor_class
from visual_foresight_amd.hparams import HParams
from visual_foresight_amd.policy.cem_controllers import PixelCostController
from visual_foresight_amd.policy.cem_controllers.samplers import AutograspSampler, PhiloxAutograspSampler, CEMSampler
from visual_foresight_amd.policy.cem_controllers.samplers import philox_autograsp_sampler as pas
from visual_foresight_amd.policy.cem_controllers.samplers import philox_gaussian_sampler as pgs
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import PhiloxGaussianCEMSampler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = np.array([0.9, 0.1, 0.25, 0., 0.])
MARGIN = 1e-9


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def hp_for(cls=PhiloxAutograspSampler, **over):
    hp = HParams(replan_interval=0)
    for k, v in cls.get_default_hparams().items():
        hp.add_hparam(k, v)
    for k, v in over.items():
        if k in hp:
            setattr(hp, k, v)
        else:
            hp.add_hparam(k, v)
    return hp


def make(adim=4, **over):
    over.setdefault('sampler_seed', 1234)
    return PhiloxAutograspSampler(hp_for(**over), adim, 5)


# ----------------------------------------------------------------------------- hyper-parameters and the width
def test_hyper_parameters_are_the_parents_plus_the_reference_seven():
    ours, parent, ref = (c.get_default_hparams() for c in (PhiloxAutograspSampler, PhiloxGaussianCEMSampler, AutograspSampler))
    assert set(ours) == set(parent) | set(pas.GRIP_HPARAMS) and len(pas.GRIP_HPARAMS) == 7
    assert all(ours[k] == parent[k] for k in parent) and all(ours[k] == ref[k] for k in pas.GRIP_HPARAMS)
    s = make(adim=5)
    assert s._adim == 4 and s.action_width() == 5 and s.device_cem_driver == 'DeviceAutograspCEM'
    # every other sampler emits what it proposes over
    assert CEMSampler(None, 4, 5).action_width() == 4
    assert PhiloxGaussianCEMSampler(hp_for(PhiloxGaussianCEMSampler, sampler_seed=1), 4, 5).action_width() == 4


# ----------------------------------------------------------------------------- the moves
@pytest.mark.parametrize('over', [dict(), dict(rejection_sampling=False, add_zero_action=True, discrete_ind=[3]),
                                  dict(repeat=1, nactions=7)])
def test_moves_are_the_gaussian_twins_bit_for_bit(over):
    """First proposal and two refits, with and without rejection: columns 0 .. adim - 2 equal those of a
    ``PhiloxGaussianCEMSampler(hp, adim - 1, sdim)`` with the same key and call numbers."""
    adim, M, K = 5, 24, 6
    hp = hp_for(sampler_seed=77, **over)
    s, g = PhiloxAutograspSampler(hp, adim, 5), PhiloxGaussianCEMSampler(hp, adim - 1, 5)
    assert s.key == g.key
    with quiet():
        a, b = s.sample_initial_actions(0, M, STATE), g.sample_initial_actions(0, M, STATE)
    for refit in range(3):
        assert a.shape == (M, hp.nactions * hp.repeat, adim) and a.dtype == np.float64
        np.testing.assert_array_equal(a[:, :, :adim - 1], b)
        np.testing.assert_array_equal(s.last_trials, g.last_trials)
        assert s.last_margin == g.last_margin and s._call == g._call == refit + 1
        elites = pgs.select_elites(np.random.RandomState(refit).normal(size=M), K)
        a = s.sample_next_actions(M, a[elites], np.zeros(K))
        b = g.sample_next_actions(M, b[elites], np.zeros(K))
        np.testing.assert_array_equal(s._A, g._A)
    assert s.n_capped == g.n_capped


# ----------------------------------------------------------------------------- the gripper by height
@pytest.mark.parametrize('reopen', [False, True])
@pytest.mark.parametrize('over', [dict(), dict(action_norm_factor=0.37, gripper_close_cmd=0.75, gripper_open_cmd=-0.5, z_thresh=0.2)])
def test_gripper_by_height_is_the_references(reopen, over):
    """With ``deviation_prob`` 0 the column equals ``AutograspSampler._sample_gripper``'s on the same float32-representable
    moves."""
    M, T = 50, 15
    moves32 = np.random.RandomState(3).normal(0, 0.08, (M, T, 3)).astype(np.float32)
    hp = hp_for(reopen=reopen, **over)
    ref = AutograspSampler(hp_for(AutograspSampler, reopen=reopen, **over), 4, 5)
    ref._current_state = STATE
    want = ref._sample_gripper(moves32.astype(np.float64), M)
    got, below, latched = pas.gripper_from_moves(moves32, STATE[2], hp, (1, 2), 0, np.arange(M), with_latched=True)
    assert got.dtype == np.float32 and got.shape == (M, T)
    np.testing.assert_array_equal(got.astype(np.float64), want[:, :, 3])
    assert sorted(np.unique(got)) == sorted(np.float32([hp.gripper_open_cmd, hp.gripper_close_cmd]))
    assert (below != latched).any() != reopen           # the latch changed a step exactly when it applies
    with pytest.raises(TypeError):
        pas.gripper_from_moves(moves32.astype(np.float64), STATE[2], hp, (1, 2), 0, np.arange(M))


def test_heights_are_summed_in_order_each_operation_rounded_once():
    hp = hp_for(action_norm_factor=0.3)
    moves32 = np.random.RandomState(4).normal(0, 0.1, (3, 70, 3)).astype(np.float32)
    h = pas.heights(moves32, 0.21, hp)
    for i in range(3):
        c = None
        for t in range(70):
            p = float(moves32[i, t, 2]) * 0.3
            c = p if c is None else c + p
            assert h[i, t] == c + 0.21
    assert pas.grip_margin(moves32, 0.21, hp) == np.abs(h - 0.15).min()


def test_sampler_derives_the_gripper_from_its_float32_moves():
    s = make(sampler_seed=5, deviation_prob=0.25)
    with quiet():
        a = s.sample_initial_actions(0, 30, STATE)
    moves32 = a[:, :, :3].astype(np.float32)
    want = pas.gripper_from_moves(moves32, STATE[2], s._hp, s.key, 0, np.arange(30))
    np.testing.assert_array_equal(a[:, :, 3], want.astype(np.float64))
    assert s.last_grip_margin == pas.grip_margin(moves32, STATE[2], s._hp) and s.state_z() == 0.25
    b = s.sample_next_actions(30, a[:8], np.zeros(8))           # no_refit: by height again, call 1
    np.testing.assert_array_equal(b[:, :, 3], pas.gripper_from_moves(b[:, :, :3].astype(np.float32), STATE[2], s._hp, s.key, 1,
                                                                     np.arange(30)).astype(np.float64))


# ----------------------------------------------------------------------------- the uniforms
def test_uniform_words_are_those_of_the_gripper_trial():
    key, call, T = (7, 9), 3, 11
    u = pas.grip_uniforms(key, call, [4, 20], T)
    assert u.shape == (2, T) and pas.GRIP_TRIAL == 0xFFFFFFFE
    for row, i in enumerate((4, 20)):
        for t in range(T):
            w = pgs.philox4x32_10(np.array([t // 4, 0xFFFFFFFE, i, call]), key)
            assert u[row, t] == float(w[t % 4]) / 2.0 ** 32


def test_deviation_flips_after_the_latch_and_zero_draws_nothing(monkeypatch):
    M, T = 40, 15
    moves32 = np.random.RandomState(6).normal(0, 0.08, (M, T, 3)).astype(np.float32)
    idx = np.arange(M) + 3
    plain, _, latched = pas.gripper_from_moves(moves32, 0.25, hp_for(), (1, 2), 2, idx, with_latched=True)
    flipped = pas.gripper_from_moves(moves32, 0.25, hp_for(deviation_prob=0.3), (1, 2), 2, idx)
    u = pas.grip_uniforms((1, 2), 2, idx, T)
    np.testing.assert_array_equal(flipped == 1, np.logical_xor(latched, u < 0.3))
    assert 0.2 < (flipped != plain).mean() < 0.4

    def no_draw(*a, **k):
        raise AssertionError('deviation_prob 0 draws no uniform')
    monkeypatch.setattr(pas, 'grip_uniforms', no_draw)
    np.testing.assert_array_equal(pas.gripper_from_moves(moves32, 0.25, hp_for(), (1, 2), 2, idx), plain)
    with quiet():
        make(sampler_seed=8).sample_initial_actions(0, 10, STATE)


# ----------------------------------------------------------------------------- the gripper by the elites' share
def test_share_branch_is_the_references_mean_and_the_stated_words():
    s = make(sampler_seed=9, no_refit=False, gripper_close_cmd=0.75, gripper_open_cmd=-0.5)
    M, K = 40, 7
    with quiet():
        a = s.sample_initial_actions(0, M, np.array([0., 0., 0.3, 0., 0.]))
    elites = a[pgs.select_elites(np.random.RandomState(1).normal(size=M), K)]
    elites[:, 0, 3], elites[:, -1, 3] = -0.5, 0.75              # a share of 0 and a share of 1
    b = s.sample_next_actions(M, elites, np.zeros(K))
    want_share = np.mean((elites[:, :, -1] == 0.75).astype(np.float32), axis=0)
    assert s.last_share.dtype == np.float32
    np.testing.assert_array_equal(s.last_share, want_share)
    assert want_share[0] == 0 and want_share[-1] == 1 and ((want_share > 0) & (want_share < 1)).any()
    u = pas.grip_uniforms(s.key, 1, np.arange(M), a.shape[1])
    np.testing.assert_array_equal(b[:, :, 3] == 0.75, u < want_share[None].astype(np.float64))
    assert set(np.unique(b[:, :, 3])) == {-0.5, 0.75} and (b[:, 0, 3] == -0.5).all() and (b[:, -1, 3] == 0.75).all()
    assert s.last_grip_margin == np.inf and s.by_share(1) and not s.by_share(0) and not make().by_share(1)
    # the moves of the refit are still the parent's
    g = PhiloxGaussianCEMSampler(s._hp, 3, 5)
    g._call = 1
    g.refit(elites[:, :, :3])
    np.testing.assert_array_equal(b[:, :, :3], g._sample(M))


# ----------------------------------------------------------------------------- refusals
def test_constructor_refusals():
    with pytest.raises(ValueError, match='3 move channels'):
        make(adim=3)
    with pytest.raises(ValueError, match='exceeds 8'):
        make(adim=5, append_action=[0.0] * 4)
    make(adim=5, append_action=[0.0] * 3)
    with pytest.raises(ValueError, match='max_trials'):
        make(max_trials=0xFFFFFFFE)
    with pytest.raises(ValueError, match='deviation_prob'):
        make(deviation_prob=1.5)
    for name in ('reuse_cov', 'smooth_cov', 'cov_blockdiag'):
        with pytest.raises(ValueError, match=name):
            make(**{name: True})
    with pytest.raises(ValueError):
        make(adim=5, nactions=33)           # D = 132
    with pytest.raises(ValueError):
        make(max_trials=0)


# ----------------------------------------------------------------------------- one planning call on the host route
def test_one_act_of_the_pixel_cost_controller_takes_the_host_route():
    T, H, W = 15, 16, 16
    fake = make_fake_predictor_class(T, H, W)
    seen = []

    class Recording(PhiloxAutograspSampler):
        def sample_next_actions(self, n_samples, best_actions, scores):
            seen.append(np.array(best_actions))
            return super(Recording, self).sample_next_actions(n_samples, best_actions, scores)

    pol = dict(predictor_class=fake, verbose=False, sampler=Recording, num_samples=40, sampler_seed=11, no_refit=False)   # (iterations: 3)
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    rs = np.random.RandomState(1)
    images, states = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8), rs.normal(0.2, 0.05, (2, 5))
    with quiet():
        ctrl = PixelCostController(ag, dict(pol), 0, 1)
        ctrl.reset()
        assert ctrl._device_cem_plan() is None          # (the stand-in predictor has no device entry)
        out = ctrl.act(t=1, i_tr=0, desig_pix=[[8, 8]], goal_pix=[[3, 12]], images=images, state=states)
    assert isinstance(ctrl._sampler, PhiloxAutograspSampler) and ctrl._hp.device_cem is True
    assert out['actions'].shape == (4,) and sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
    assert len(seen) == 2 and all(e.shape == (10, T, 4) for e in seen)
    assert all(set(np.unique(e[:, :, 3])) <= {-1.0, 1.0} for e in seen)
    np.testing.assert_array_equal(ctrl._sampler.last_share, pas.elite_share(seen[1], ctrl._hp, 3))
    np.testing.assert_array_equal(ctrl._best_indices, pgs.select_elites(out['plan_stat']['scores_itr2'], 10))
    np.testing.assert_array_equal(out['actions'], ctrl._best_actions[0, 0])
    assert ctrl._sampler._call == 3 and ctrl._sampler.state_z() == states[-1, 2]


# ----------------------------------------------------------------------------- the library
def test_library_exports_the_autograsp_entry():
    from visual_foresight_amd import _lib
    from visual_foresight_amd.policy.cem_controllers.device_cem import autograsp_config, grip_config
    header = open(os.path.join(REPO, 'include', 'vf_hip.h')).read()
    assert set(re.findall(r'\b(vf_[a-z_]+)\s*\(', header)) == set(_lib.EXPORTS)
    assert re.search(r'\bint vf_cem_sample_autograsp\(', header) and 'vf_cem_sample_autograsp' in _lib.EXPORTS
    _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, 'vf_cem_sample_autograsp') and lib.vf_abi_version() == 7
    s = make(adim=5, append_action=[0.25])
    s.start_planning_call(STATE)
    cfg, grip = autograsp_config(s, 10, [0.25]), grip_config(s, False)
    assert (cfg.adim, cfg.tail, cfg.tail_value[1]) == (4, 2, 0.25) and (grip.mode, grip.state_z) == (0, 0.25)
    assert lib.vf_cem_workspace_bytes(ctypes.byref(cfg)) == 16 + 8 * 20 * 21
    # refusals need no device: nothing is launched
    assert lib.vf_cem_sample_autograsp(0, ctypes.byref(cfg), ctypes.byref(grip), None, 0, 4, None, None, None, None, None,
                                       None) == -1
    assert b'vf_cem_sample_autograsp' in lib.vf_last_error()


# ----------------------------------------------------------------------------- the seeds of the GPU cases
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_seeds_keep_clear_of_every_boundary(name):
    """(CPU) No value the twin tests lies within 1e-9 of a rejection limit, and no planned height within
    ``T * action_norm_factor * 2**-23 * max|lift|`` of ``z_thresh`` - what one float32 ulp per step can move a height: an ulp
    of the device's log / sin / cos cannot flip a decision for these seeds.  Every case emits both commands; the latch cases
    hold a step the latch changes; the share case holds shares of 0, of 1 and in between."""
    want = cases.twin_run(name)
    M, K, nactions, repeat, adim = cases.CASES[name][:5]
    s, T = want['sampler'], nactions * repeat
    hp = s._hp
    assert want['margin'] > MARGIN
    seen, changed = set(), 0
    for call, actions in enumerate(want['calls']):
        assert actions.shape == (M, T, adim + len(want['tail'] or ()))
        seen |= set(np.unique(actions[:, :, adim - 1]).tolist())
        if want['share'][call] is None:
            bound = T * hp.action_norm_factor * 2.0 ** -23 * want['max_lift'][call]
            assert want['grip_margin'][call] > bound, (call, want['grip_margin'][call], bound)
            _, below, latched = pas.gripper_from_moves(actions[:, :, :adim - 1].astype(np.float32), s.state_z(), hp, s.key, call,
                                                       np.arange(M), with_latched=True)
            changed += int((below != latched).sum())
    assert seen == {float(np.float32(hp.gripper_close_cmd)), float(np.float32(hp.gripper_open_cmd))}
    if name in cases.LATCHED:
        assert changed > 0
    if name == 'reopen':
        assert changed == 0
    if name == 'share':
        for share in want['share'][1:]:
            assert (share == 0).any() and (share == 1).any() and ((share > 0) & (share < 1)).any()
    if name == 'capped':
        assert want['n_capped'] == 3 * M
    if name == 'no_rejection':
        assert all((c[0, :, :adim - 1] == 0).all() and (c[0, :, adim - 1] == 1).all() for c in want['calls'])
