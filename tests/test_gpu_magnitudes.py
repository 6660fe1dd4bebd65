"""The LayerNorm predictors (arch 'cdna', 'savp', 'savp2') at the magnitudes of a trained checkpoint, and in closed form.

Every other GPU test runs Glorot weights with tiny biases: raw pre-LayerNorm outputs below 3, gates near zero, a flat mask
softmax.  Here (networks, inputs and their CPU-side conditions: tests/helpers/weight_regimes.py, tests/test_weight_regimes.py):

a. raw layers scaled by powers of two, so that waves of one sample sit on BOTH branches of the exact LayerNorm statistics
   (float64 sums below |v| = 128, per-value integers above: vf_fused_top.h, vf_conv_first.h) - against the float32 oracle,
   at the tolerances of test_gpu_parity.py / test_gpu_savp.py;
b. the same networks through every launch strategy: the fused top, the per-layer EPI_CONVT_RAW_STATS launch and the
   stand-alone compositing tile cut one layer into different waves, hence into different branches - same bits;
c. gates, heads and CDNA kernels saturated through their biases (sigmoid / tanh / softmax at +-100, the relu shift);
d. a copy and a shift network, whose rollout is known without any oracle.

Designated pixels are drawn as (row in [0, H), column in [0, W)); tasks sit at (0, 0), (H - 1, W - 1), (0, W - 1) and, at
48 x 64, in a column beyond H; goals lie on and off the image.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                              # noqa: E402
from tests.helpers import weight_regimes as wr             # noqa: E402

FINAL_WEIGHT = 10.
PARITY_RAW = [n for n, c in wr.RAW_CASES.items() if c['kind'] == 'parity']
BITS_RAW = [n for n, c in wr.RAW_CASES.items() if c['kind'] == 'bits']


def _predictor(weights, bs, **extra):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    cfg = weights.cfg
    hp = dict(designated_pixel_count=cfg.ndesig, run_batch_size=bs, adim=cfg.adim, sdim=cfg.sdim, image_height=cfg.height,
              image_width=cfg.width, sequence_length=cfg.sequence_length, arch=cfg.arch, **extra)
    if getattr(cfg, 'decoder', 'survey') != 'survey':
        hp['decoder'] = cfg.decoder
    pred = HipVPredEvaluation('', hp)
    pred.restore(weights)
    return pred


def _device(pred, ctx, actions, goal):
    scores, per_task = pred.score(ctx, {'actions': actions}, goal, finalweight=FINAL_WEIGHT)
    got = pred(ctx, {'actions': actions})
    assert pred.device_status() == 0
    return scores, per_task, got['predicted_frames'], got['predicted_pixel_distributions'], got['predicted_states']


@functools.lru_cache(maxsize=None)
def _oracles(kind, name):
    """The case with its float32 and float64 rollouts: computed once, shared, never written to."""
    weights, ctx, actions, goal = (wr.raw_case if kind == 'raw' else wr.saturated_case)(name)
    out = [weights, ctx, actions, goal]
    for dtype in (torch.float32, torch.float64):
        out.append(wr.rollout(wr.oracle_for(weights, dtype), ctx, actions))
    return tuple(out)


def _distances(frames, distrib, f64, d64):
    return (float(np.abs(frames - f64).max()), float((np.abs(distrib - d64) / d64.max(axis=(3, 4), keepdims=True)).max()))


def _assert_parity(label, dev, goal, o32, o64):
    """The assertions of test_rollout_matches_oracle / test_savp_rollout_matches_oracle, against the float32 oracle."""
    scores, per_task, frames, distrib, states = dev
    f, d, s = o32
    e_dev, e_ora = _distances(frames, distrib, *o64[:2]), _distances(f, d, *o64[:2])
    print('%s vs float64: device frames %.2e distributions %.2e | float32 oracle frames %.2e distributions %.2e'
          % (label, e_dev[0], e_dev[1], e_ora[0], e_ora[1]))
    for x in dev:
        assert np.isfinite(x).all()
    assert np.abs(frames - f).max() <= 1e-5
    assert (np.abs(distrib - d) / d.max(axis=(3, 4), keepdims=True)).max() <= 2e-5
    assert np.abs(states - s).max() <= 1e-6
    want, want_pt = pixel_cost.eval_pixel_cost(d, goal, FINAL_WEIGHT)
    np.testing.assert_allclose(scores, want, rtol=1e-5)
    np.testing.assert_allclose(per_task, want_pt, rtol=1e-5)
    own, _ = pixel_cost.eval_pixel_cost(distrib, goal, FINAL_WEIGHT)
    np.testing.assert_allclose(scores, own, rtol=2e-6)


def _assert_strategies_give_the_same_bits(weights, ctx, actions, goal, **extra):
    M = len(actions)
    pred = _predictor(weights, M, **extra)
    base = _device(pred, ctx, actions, goal)
    toggles = (('persistent', pred.set_persistent), ('xcd_queues', pred.set_xcd_queues), ('dedup', pred.set_dedup),
               ('fuse_top', pred.set_fuse_top), ('write_through', lambda v: pred.set_sched_option('write_through', v)))
    for label, switch in toggles:
        switch(0)
        pred._ctx_key = None                # upload the context again: this variant computes the shared units itself
        for a, b in zip(base, _device(pred, ctx, actions, goal)):
            np.testing.assert_array_equal(a, b, err_msg=label + ' = 0')
        switch(1)
    pred._ctx_key = None
    perm = np.random.RandomState(M).permutation(M)
    for a, b in zip(base, _device(pred, ctx, actions[perm], goal)):
        np.testing.assert_array_equal(a[perm], b, err_msg='permutation')
    ragged = _predictor(weights, 9, **extra)            # chunks of 9, the last one ragged
    for a, b in zip(base, _device(ragged, ctx, actions, goal)):
        np.testing.assert_array_equal(a, b, err_msg='run_batch_size = 9')


# ------------------------------------------------------------------------------------------------ a. raw-scaled parity
@pytest.mark.parametrize('name', PARITY_RAW)
def test_raw_scaled_rollout_matches_oracle(name):
    weights, ctx, actions, goal, o32, o64 = _oracles('raw', name)
    pred = _predictor(weights, len(actions))
    _assert_parity('raw-scaled %s' % name, _device(pred, ctx, actions, goal), goal, o32, o64)


# ------------------------------------------------------------------------------------------------ b. raw-scaled bit identity
@pytest.mark.parametrize('name', BITS_RAW)
def test_raw_scaled_launch_strategies_are_bit_identical(name):
    weights, ctx, actions, goal = wr.raw_case(name)
    assert len(actions) == 37
    _assert_strategies_give_the_same_bits(weights, ctx, actions, goal)


# ------------------------------------------------------------------------------------------------ c. bias-saturated
@pytest.mark.parametrize('name', list(wr.SATURATED_CASES))
def test_bias_saturated_rollout_matches_oracle(name):
    weights, ctx, actions, goal, o32, o64 = _oracles('saturated', name)
    pred = _predictor(weights, len(actions))
    _assert_parity('bias-saturated %s' % name, _device(pred, ctx, actions, goal), goal, o32, o64)


def test_bias_saturated_split_bf16_mode_has_fp32_class_accuracy():
    """The rule of test_split_bf16_mode_has_fp32_class_accuracy on the saturated network: precision='bf16x6' within 4x of
    the distance of the exact-fp32 path to the float64 oracle, and inside the fp32 tolerances."""
    weights, ctx, actions, goal, _, (f, d, _s) = _oracles('saturated', 'cdna-32')
    want, _ = pixel_cost.eval_pixel_cost(d.astype(np.float32), goal, FINAL_WEIGHT)
    errs = {}
    for prec in ('fp32', 'bf16x6'):
        for persistent in (1, 0):
            pred = _predictor(weights, len(actions), precision=prec)
            pred.set_persistent(persistent)
            dev = _device(pred, ctx, actions, goal)
            for x in dev:
                assert np.isfinite(x).all()
            errs[(prec, persistent)] = _distances(dev[2], dev[3], f, d) + (float(np.abs(dev[0] / want - 1).max()),)
    print('bias-saturated cdna-32 bf16x6 vs float64 (frames, distributions, scores): fp32 %s | bf16x6 %s'
          % (' '.join('%.2e' % e for e in errs[('fp32', 1)]), ' '.join('%.2e' % e for e in errs[('bf16x6', 1)])))
    for persistent in (1, 0):
        e32, e16 = errs[('fp32', persistent)], errs[('bf16x6', persistent)]
        assert e16[0] <= 1e-5 and e16[1] <= 2e-5 and e16[2] <= 1e-5
        assert e16[0] <= 4 * e32[0] + 1e-7 and e16[1] <= 4 * e32[1] + 1e-7, (e32, e16)
    assert errs[('bf16x6', 1)] == errs[('bf16x6', 0)]


def test_bias_saturated_launch_strategies_are_bit_identical():
    weights, ctx, _, goal = wr.saturated_case('cdna-48x64-starved')
    actions = np.random.RandomState(37).normal(0, 0.1, (37, 2, weights.cfg.adim))
    _assert_strategies_give_the_same_bits(weights, ctx, actions, goal)


# ------------------------------------------------------------------------------------------------ d. closed form
@pytest.mark.parametrize('persistent', [1, 0])
@pytest.mark.parametrize('name', list(wr.CLOSED_CASES))
def test_copy_network_repeats_the_last_context_frame(name, persistent):
    weights, ctx, actions, goal, pixels = wr.closed_case(name, 'copy')
    T = wr.CLOSED_CASES[name]['T']
    pred = _predictor(weights, len(actions), persistent=persistent)
    scores, per_task, frames, distrib, _ = _device(pred, ctx, actions, goal)
    want = wr.closed_form_frames(ctx, 'copy', None, T)
    assert np.abs(frames[:, :, 0] - want[None]).max() <= 1e-30       # the other masks are <= e^-80: denormal residue at most
    assert (scores == scores[0]).all()
    want_score, want_pt = wr.closed_form_scores(pixels, goal, FINAL_WEIGHT)
    np.testing.assert_allclose(per_task, np.tile(want_pt, (len(actions), 1)), rtol=2e-6)
    np.testing.assert_allclose(scores, want_score, rtol=2e-6)
    for p in range(pixels.shape[1]):
        plane = distrib[:, :, 0, :, :, p].reshape(len(actions), T, -1)
        assert (plane.argmax(-1) == pixels[None, :, p, 0] * weights.cfg.width + pixels[None, :, p, 1]).all()


@pytest.mark.parametrize('persistent', [1, 0])
@pytest.mark.parametrize('tap', wr.SHIFT_TAPS)
@pytest.mark.parametrize('name', list(wr.CLOSED_CASES))
def test_shift_network_moves_frames_and_pixels_by_its_tap(name, tap, persistent):
    weights, ctx, actions, goal, pixels = wr.closed_case(name, 'shift', tap)
    T = wr.CLOSED_CASES[name]['T']
    pred = _predictor(weights, len(actions), persistent=persistent)
    scores, per_task, frames, distrib, _ = _device(pred, ctx, actions, goal)
    want = wr.closed_form_frames(ctx, 'shift', tap, T)
    for t in range(T):      # one float32 ulp of 1.0 per step + the float64 oracle's own distance to the closed form
        err = np.abs(frames[:, t, 0] - want[None, t]).max()
        assert err <= (t + 1) * 2. ** -23 + wr.CLOSED_FORM_ORACLE_BOUND, (t, err)
    for p in range(pixels.shape[1]):
        plane = distrib[:, :, 0, :, :, p].reshape(len(actions), T, -1)
        assert (plane.argmax(-1) == pixels[None, :, p, 0] * weights.cfg.width + pixels[None, :, p, 1]).all()
    want_score, want_pt = wr.closed_form_scores(pixels, goal, FINAL_WEIGHT)
    np.testing.assert_allclose(per_task, np.tile(want_pt, (len(actions), 1)), rtol=2e-6)
    np.testing.assert_allclose(scores, want_score, rtol=2e-6)
