"""The published SAVP generator (arch 'savp3') off Glorot weights, and in closed form.

Every other device test of it runs ``CdnaWeights.random(..., bias_scale=0.05, ln_jitter=0.1)``: instance-norm variances 1e5
times the epsilon, conditioning tables that carry a few percent of a layer, a flat mask softmax, maps with an interior
border class.  Here (networks, inputs, closed forms: tests/helpers/savp3_regimes.py; their CPU-side conditions:
tests/test_savp3_regimes.py):

a. parity with the float32 oracle at the tolerances of test_gpu_savp3.py, plus its 3x rule against float64, with convs scaled
   down until the variance is at or below the epsilon (2^-10, 2^-14: the epsilon is a first-order term), scaled up (2^10), the
   conditioning rows x 32 on deepest maps of 4 x 4 and 4 x 5 (no interior border class), gate offsets from {-4, 0, 4};
b. regimes in which the float32 oracle itself drifts from float64 (one gain x 8, conv biases + 8 / + 32, gate offsets from
   {-8, 0, 8}, masks/w x 8): the 3x rule alone;
c. the launch strategies at these magnitudes: same bits;
d. each of the seven compositing slots at +100: the rollout is known in NumPy without any oracle - slot order, symmetric
   padding, the distribution path's own slots, the all-taps-dead box mean, sigmoid at +-100.

Designated pixels are drawn as (row in [0, H), column in [0, W)) and sit at (0, 0), (H - 1, W - 1), (0, W - 1) among others;
goals lie on and off the image.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                              # noqa: E402
from tests.helpers import savp3_regimes as s3              # noqa: E402
from tests.helpers.weight_regimes import closed_form_scores   # noqa: E402

FW = s3.FINAL_WEIGHT
ULP1 = 2. ** -23            # one float32 ulp of 1.0


def _predictor(weights, bs, **extra):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    views = weights if isinstance(weights, list) else [weights]
    cfg = views[0].cfg
    hp = dict(designated_pixel_count=cfg.ndesig, run_batch_size=bs, adim=cfg.adim, sdim=cfg.sdim, image_height=cfg.height,
              image_width=cfg.width, sequence_length=cfg.sequence_length, arch='savp3', zdim=cfg.zdim,
              layer_spec=cfg.layer_spec, ncam=len(views), **extra)
    pred = HipVPredEvaluation('', hp)
    pred.restore(weights)
    return pred


def _device(pred, ctx, actions, goal):
    scores, per_task = pred.score(ctx, {'actions': actions}, goal, finalweight=FW)
    got = pred(ctx, {'actions': actions})
    assert pred.device_status() == 0
    return scores, per_task, got['predicted_frames'], got['predicted_pixel_distributions'], got['predicted_states']


@functools.lru_cache(maxsize=None)
def _oracles(name):
    """The case (PARITY_M samples) with its float32 and float64 rollouts: computed once, shared, never written to."""
    weights, ctx, actions, goal = s3.case(name)
    out = [weights, ctx, actions, goal]
    for dtype in (torch.float32, torch.float64):
        out.append(s3.rollout(s3.oracle_for(weights, dtype), ctx, actions))
    return tuple(out)


def _distances(frames, distrib, f64, d64):
    return (float(np.abs(frames - f64).max()), float((np.abs(distrib - d64) / d64.max(axis=(3, 4), keepdims=True)).max()))


def _assert_three_times_rule(label, dev, goal, o32, o64, scores_too=False):
    """test_hip_is_as_close_to_float64_as_the_float32_oracle: device distance <= 3 x the float32 oracle's + 2e-6."""
    scores, _, frames, distrib, _ = dev
    e_dev, e_ora = _distances(frames, distrib, *o64[:2]), _distances(o32[0], o32[1], *o64[:2])
    want64 = pixel_cost.eval_pixel_cost(o64[1], goal, FW)[0]
    s_dev = float(np.abs(scores / want64 - 1).max())
    s_ora = float(np.abs(pixel_cost.eval_pixel_cost(o32[1], goal, FW)[0] / want64 - 1).max())
    print('%s vs float64: device frames %.2e distributions %.2e scores %.2e | float32 oracle frames %.2e distributions %.2e '
          'scores %.2e' % (label, e_dev[0], e_dev[1], s_dev, e_ora[0], e_ora[1], s_ora))
    for x in dev:
        assert np.isfinite(x).all()
    assert e_dev[0] <= 3 * e_ora[0] + 2e-6, (e_dev, e_ora)
    assert e_dev[1] <= 3 * e_ora[1] + 2e-6, (e_dev, e_ora)
    if scores_too:
        assert s_dev <= 3 * s_ora + 2e-6, (s_dev, s_ora)


def _assert_parity(label, dev, goal, o32, o64):
    """The assertions of test_savp3_rollout_matches_oracle against the float32 oracle, and the 3x rule against float64."""
    _assert_three_times_rule(label, dev, goal, o32, o64)
    scores, per_task, frames, distrib, states = dev
    f, d, s = o32
    assert np.abs(frames - f).max() <= 3e-5
    assert (np.abs(distrib - d) / d.max(axis=(3, 4), keepdims=True)).max() <= 2e-5
    assert np.abs(states - s).max() <= 1e-6
    want, want_pt = pixel_cost.eval_pixel_cost(d, goal, FW)
    np.testing.assert_allclose(scores, want, rtol=1e-5)
    np.testing.assert_allclose(per_task, want_pt, rtol=1e-5)
    np.testing.assert_allclose(distrib.sum(axis=(3, 4)), 1.0, atol=5e-6)


# ------------------------------------------------------------------------------------------------ a. well-conditioned parity
@pytest.mark.parametrize('name', s3.WELL)
def test_well_conditioned_regime_matches_oracle(name):
    weights, ctx, actions, goal, o32, o64 = _oracles(name)
    pred = _predictor(weights, len(actions))
    _assert_parity(name, _device(pred, ctx, actions, goal), goal, o32, o64)


# ------------------------------------------------------------------------------------------------ b. ill-conditioned: 3x rule
@pytest.mark.parametrize('name', s3.ILL)
def test_ill_conditioned_regime_is_as_close_to_float64_as_the_float32_oracle(name):
    weights, ctx, actions, goal, o32, o64 = _oracles(name)
    pred = _predictor(weights, len(actions))
    _assert_three_times_rule(name, _device(pred, ctx, actions, goal), goal, o32, o64, scores_too=True)


# ------------------------------------------------------------------------------------------------ c. launch strategies
@pytest.mark.parametrize('name', s3.BITS)
def test_launch_strategies_are_bit_identical_at_these_magnitudes(name):
    weights, ctx, actions, goal = s3.case(name, M=s3.BITS_M)
    M = len(actions)
    assert M == 23
    pred = _predictor(weights, M)
    base = _device(pred, ctx, actions, goal)
    for kw in (dict(persistent=0), dict(xcd_queues=0), dict(run_batch_size=9), dict(run_batch_size=1)):
        hp = dict(kw)
        other = _predictor(weights, hp.pop('run_batch_size', M), **hp)
        for a, b in zip(base, _device(other, ctx, actions, goal)):
            np.testing.assert_array_equal(a, b, err_msg=str(kw))
    pred.set_sched_option('write_through', 0)
    for a, b in zip(base, _device(pred, ctx, actions, goal)):
        np.testing.assert_array_equal(a, b, err_msg='write_through = 0')
    pred.set_sched_option('write_through', 1)
    perm = np.random.RandomState(M).permutation(M)
    for a, b in zip(base, _device(pred, ctx, actions[perm], goal)):
        np.testing.assert_array_equal(a[perm], b, err_msg='permutation')
    for a, b in zip(base, _device(pred, ctx, actions, goal)):
        np.testing.assert_array_equal(a, b, err_msg='second run')
    # the four-phase heads are another summation order: parity on their own (the oracles hold the first PARITY_M samples)
    _, _, _, _, o32, o64 = _oracles(name)
    n = s3.PARITY_M
    unfused = _predictor(weights, n, fuse_top=0)
    _assert_parity(name + ' fuse_top = 0', _device(unfused, ctx, actions[:n], goal), goal, o32, o64)
    for a, b in zip(base, _device(pred, ctx, actions[:n], goal)):           # (and the fused ones on the same samples)
        np.testing.assert_array_equal(a[:n], b)


# ------------------------------------------------------------------------------------------------ d. closed forms
def _assert_distributions(distrib, want_d, bound=2e-6):
    """distrib [M, T, H, W, nd] against the closed form [T, H, W, nd], over plane max."""
    err = np.abs(distrib - want_d[None]) / want_d.max(axis=(1, 2), keepdims=True)[None]
    assert err.max() <= bound, err.max()


def _assert_same_for_every_sample(scores, per_task):
    assert (scores == scores[0]).all() and (per_task == per_task[0]).all()


@pytest.mark.parametrize('persistent', [1, 0])
@pytest.mark.parametrize('slot', [s3.SLOT_PREV, s3.SLOT_FIRST])
def test_background_slots_repeat_the_last_and_the_first_context_frame(slot, persistent):
    weights, ctx, actions, goal, _ = s3.closed_case(slot, 'corner')
    scores, per_task, frames, distrib, _ = _device(_predictor(weights, len(actions), persistent=persistent), ctx, actions, goal)
    want_f, want_d = s3.closed_form(ctx, s3.closed_kind(slot), s3.CLOSED_T)
    assert np.abs(frames[:, :, 0] - want_f[None]).max() <= 1e-30          # the other masks are below e^-90
    _assert_distributions(distrib[:, :, 0], want_d)
    _assert_same_for_every_sample(scores, per_task)
    want = pixel_cost.eval_pixel_cost(np.broadcast_to(want_d[None, :, None], distrib.shape), goal, FW)
    np.testing.assert_allclose(scores, want[0], rtol=2e-6)
    np.testing.assert_allclose(per_task, want[1], rtol=2e-6)


@pytest.mark.parametrize('persistent', [1, 0])
def test_scratch_slot_paints_the_saturated_scratch_image_and_keeps_the_distribution(persistent):
    """sigmoid(+-100) must be exactly 1 and 0 (exp overflows), sigmoid(0) one half; the distribution path's slot 6 carries
    the PREVIOUS distribution, not the scratch image."""
    weights, ctx, actions, goal, _ = s3.closed_case(s3.SLOT_SCRATCH, 'corner')
    scores, per_task, frames, distrib, _ = _device(_predictor(weights, len(actions), persistent=persistent), ctx, actions, goal)
    want_f, want_d = s3.closed_form(ctx, 'scratch', s3.CLOSED_T)
    assert np.abs(want_f[0, 0, 0] - np.array([1., 0., .5])).max() <= 1e-40
    assert np.abs(frames[:, :, 0] - want_f[None]).max() <= ULP1
    _assert_distributions(distrib[:, :, 0], want_d)
    _assert_same_for_every_sample(scores, per_task)


@pytest.mark.parametrize('persistent', [1, 0])
@pytest.mark.parametrize('tap', s3.SHIFT_TAPS)
@pytest.mark.parametrize('slot', [0, 1, 2, 3])
def test_warp_slots_shift_frames_and_pixels_by_their_own_kernels_tap(slot, tap, persistent):
    """Kernel ``slot`` is one tap, the other three kernels the mirrored tap: the frames are the symmetric-pad shift by THIS tap."""
    pred = None
    for context in s3.CLOSED_CONTEXTS:
        weights, ctx, actions, goal, pix = s3.closed_case(slot, context, tap)
        if pred is None:
            pred = _predictor(weights, len(actions), persistent=persistent)
        scores, per_task, frames, distrib, _ = _device(pred, ctx, actions, goal)
        want_f, want_d = s3.closed_form(ctx, 'warp', s3.CLOSED_T, tap)
        for t in range(s3.CLOSED_T):      # one float32 ulp of 1.0 per step + the float64 oracle's own distance to the closed form
            err = np.abs(frames[:, t, 0] - want_f[None, t]).max()
            assert err <= (t + 1) * ULP1 + s3.CLOSED_FORM_ORACLE_BOUND, (context, t, err)
        flat = distrib[:, :, 0].reshape(len(actions), s3.CLOSED_T, -1, distrib.shape[-1])
        want_arg = want_d.reshape(s3.CLOSED_T, -1, want_d.shape[-1]).argmax(1)
        _assert_same_for_every_sample(scores, per_task)
        if context == 'inside':
            assert (flat.argmax(2) == want_arg[None]).all()
            pixels = s3.shifted_pixels(pix, tap, s3.CLOSED_T, s3.CLOSED_H, s3.CLOSED_W)
            assert (want_arg == pixels[..., 0] * s3.CLOSED_W + pixels[..., 1]).all()
            want_score, want_pt = closed_form_scores(pixels, goal[0], FW)
            np.testing.assert_allclose(per_task, np.tile(want_pt, (len(actions), 1)), rtol=2e-6)
            np.testing.assert_allclose(scores, want_score, rtol=2e-6)
        else:                           # the symmetric padding doubles the peak: the renormalised plane itself
            _assert_distributions(distrib[:, :, 0], want_d)


@pytest.mark.parametrize('persistent', [1, 0])
def test_dead_taps_are_a_box_mean(persistent):
    """Every tap relu(-1 - 1e-12) + 1e-12: the kernel is 1e-12 / 25e-12 everywhere.  Frames within 32 x 2^-24: 25 products and
    24 sums of values of at most 1, plus the rounding of the taps."""
    weights, ctx, actions, goal, _ = s3.closed_case(2, 'corner', dead=True, T=1)
    scores, per_task, frames, distrib, _ = _device(_predictor(weights, len(actions), persistent=persistent), ctx, actions, goal)
    want_f, want_d = s3.closed_form(ctx, 'dead', 1)
    assert np.abs(frames[:, :, 0] - want_f[None]).max() <= 32 * 2. ** -24
    _assert_distributions(distrib[:, :, 0], want_d)
    _assert_same_for_every_sample(scores, per_task)


@pytest.mark.parametrize('persistent', [1, 0])
def test_two_views_with_a_different_saturated_slot_each(persistent):
    slots = (s3.SLOT_PREV, s3.SLOT_FIRST)
    weights, ctx, actions, goal = s3.two_view_case(slots)
    scores, per_task, frames, distrib, _ = _device(_predictor(weights, len(actions), persistent=persistent), ctx, actions, goal)
    for v, slot in enumerate(slots):
        want_f, want_d = s3.closed_form(ctx, s3.closed_kind(slot), 2, view=v)
        assert np.abs(frames[:, :, v] - want_f[None]).max() <= 1e-30
        _assert_distributions(distrib[:, :, v], want_d)
    _assert_same_for_every_sample(scores, per_task)
