"""CPU-side conditions of the savp3 regimes (tests/helpers/savp3_regimes.py) that tests/test_gpu_savp3_magnitudes.py runs on
the device - float32 and float64 oracles only, no GPU:

* 'well' cases: the float32 oracle lies within a QUARTER of the device tolerances of test_gpu_savp3.py of the float64 oracle
  (frames 7.5e-6, distributions 5e-6 of plane max), so a device failure at the full tolerance is the device's;
* 'ill' cases: the float32 oracle's distance stays at or below 1e-4 - beyond that the device's 3x rule has no teeth;
* every scaled-down case moves the float64 frames by more than 0.05 against its unscaled twin: the variance is at or below the
  instance norm's epsilon, which is then a first-order term of the output (otherwise the epsilon is not being tested);
* the float64 oracle agrees with every NumPy closed form to 1e-10 (frames, distributions over plane max);
* ``Savp3Config`` and the oracle agree on the layer table of every forced-table shape.

A regime that misses its condition is given a milder factor HERE, before any device run, with the reason next to it.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle.savp3_predictor import expected_shapes                # noqa: E402
from tests.helpers import savp3_regimes as s3                      # noqa: E402
from tests.helpers import weight_regimes as wr                     # noqa: E402

WELL_FRAMES, WELL_DISTRIB = 7.5e-6, 5e-6
ILL_CAP = 1e-4
EPS_FIRST_ORDER = 0.05


def _distances(frames, distrib, f64, d64):
    return (float(np.abs(frames - f64).max()), float((np.abs(distrib - d64) / d64.max(axis=(3, 4), keepdims=True)).max()))


@functools.lru_cache(maxsize=None)
def _f64(name, unscaled=False):
    weights, ctx, actions, _ = s3.case(name, unscaled=unscaled)
    return s3.rollout(s3.oracle_for(weights, torch.float64), ctx, actions)


def _oracle_distance(name):
    weights, ctx, actions, _ = s3.case(name)
    f32, d32, _ = s3.rollout(s3.oracle_for(weights, torch.float32), ctx, actions)
    f64, d64, _ = _f64(name)
    assert np.isfinite(f32).all() and np.isfinite(d32).all()
    e = _distances(f32, d32, f64, d64)
    print('%s: float32 oracle vs float64: frames %.2e distributions %.2e' % (name, e[0], e[1]))
    return e


@pytest.mark.parametrize('name', s3.WELL)
def test_well_conditioned_cases_keep_the_float32_oracle_within_a_quarter_of_the_tolerances(name):
    e = _oracle_distance(name)
    assert e[0] <= WELL_FRAMES and e[1] <= WELL_DISTRIB, e


@pytest.mark.parametrize('name', s3.ILL)
def test_ill_conditioned_cases_stay_below_the_cap(name):
    e = _oracle_distance(name)
    assert e[0] <= ILL_CAP and e[1] <= ILL_CAP, e


@pytest.mark.parametrize('name', s3.SCALED_DOWN)
def test_epsilon_is_a_first_order_term_of_every_scaled_down_case(name):
    moved = float(np.abs(_f64(name)[0] - _f64(name, True)[0]).max())
    print('%s: float64 frames move by %.3f against the unscaled network' % (name, moved))
    assert moved > EPS_FIRST_ORDER


def test_raw_scaled_refuses_other_layers_and_factors():
    w = s3.base_weights(32, 32, 1, 2)
    assert sorted(wr.raw_layer_names(w)) == sorted(['h0c', 'h1c', 'h2c', 'h3c', 'h0l', 'h1l', 'h2l', 'hm', 'hs'])
    for bad in ({'masks': 2.}, {'scratch': 2.}, {'h0c': 3.}, {'h0l': -2.}, {'h3l': 2.}):
        with pytest.raises(ValueError):
            wr.raw_scaled(w, bad)
    out = wr.raw_scaled(w, {'h0l': 4., 'hm': 0.5})
    np.testing.assert_array_equal(out.tensors['h0l/w'], w.tensors['h0l/w'] * np.float32(4.))
    np.testing.assert_array_equal(out.tensors['hm/b'], w.tensors['hm/b'] * np.float32(0.5))
    with pytest.raises(ValueError):
        s3.cond_scaled(w, 3.)


def test_cond_scaled_touches_the_conditioning_rows_only():
    """Scaling the conditioning rows by f is feeding f times the conditioning vector: with actions, states and latents at
    zero the conditioning vector is rnn_z's output alone, and a network whose conditioning rows are zero ignores it."""
    w = s3.base_weights(32, 32, 1, 2)
    nc = w.cfg.ncond
    out = s3.cond_scaled(w, 32.)
    for name, a in w.tensors.items():
        b = out.tensors[name]
        if name.endswith('c/w') and name[0] == 'h' and name[1].isdigit():
            np.testing.assert_array_equal(b[:, :, :-nc], a[:, :, :-nc])
            np.testing.assert_array_equal(b[:, :, -nc:], a[:, :, -nc:] * np.float32(32.))
        elif name.endswith('l/w'):
            C = a.shape[3] // 4
            np.testing.assert_array_equal(b[:, :, :C], a[:, :, :C])
            np.testing.assert_array_equal(b[:, :, C + nc:], a[:, :, C + nc:])
            np.testing.assert_array_equal(b[:, :, C:C + nc], a[:, :, C:C + nc] * np.float32(32.))
        else:
            np.testing.assert_array_equal(b, a)


@pytest.mark.parametrize('H,W,spec', s3.FORCED_TABLES)
def test_config_and_oracle_agree_on_the_forced_tables(H, W, spec):
    w = s3.base_weights(H, W, 1, 2, spec)
    assert {k: tuple(v) for k, v in w.cfg.tensor_shapes().items()} == expected_shapes(w.cfg)
    f = 1 << len(w.cfg.enc)
    deepest = w.cfg.layer_table()[len(w.cfg.enc) - 1][7]
    assert deepest == (H // f, W // f) and min(deepest) == 4     # no interior border class on the short axis
    s3.oracle_for(w, torch.float32)                               # (the oracle checks the table itself)


# ---------------------------------------------------------------------------------------------------- closed forms
def _assert_closed(weights, ctx, actions, kind, tap, T):
    f64, d64, _ = s3.rollout(s3.oracle_for(weights, torch.float64), ctx, actions)
    want_f, want_d = s3.closed_form(ctx, kind, T, tap)
    ef = float(np.abs(f64[:, :, 0] - want_f[None]).max())
    ed = float((np.abs(d64[:, :, 0] - want_d[None]) / want_d.max(axis=(1, 2), keepdims=True)[None]).max())
    print('closed form %s %s: float64 oracle frames %.1e distributions %.1e' % (kind, tap, ef, ed))
    assert ef <= s3.CLOSED_FORM_ORACLE_BOUND and ed <= s3.CLOSED_FORM_ORACLE_BOUND, (ef, ed)
    return want_f, want_d


@pytest.mark.parametrize('slot', [s3.SLOT_PREV, s3.SLOT_FIRST, s3.SLOT_SCRATCH])
def test_float64_oracle_agrees_with_the_background_and_scratch_closed_forms(slot):
    weights, ctx, actions, _, _ = s3.closed_case(slot, 'corner')
    want_f, want_d = _assert_closed(weights, ctx, actions, s3.closed_kind(slot), None, s3.CLOSED_T)
    if slot == s3.SLOT_FIRST:       # the two context frames / distributions differ: slots 4 and 5 are told apart
        prev_f, prev_d = s3.closed_form(ctx, 'prev', s3.CLOSED_T)
        assert np.abs(want_f - prev_f).max() > 0.9 and np.abs(want_d - prev_d).max() > 0.4


@pytest.mark.parametrize('context', list(s3.CLOSED_CONTEXTS))
@pytest.mark.parametrize('tap', s3.SHIFT_TAPS)
@pytest.mark.parametrize('slot', [0, 1, 2, 3])
def test_float64_oracle_agrees_with_the_symmetric_shift(slot, tap, context):
    weights, ctx, actions, goal, pix = s3.closed_case(slot, context, tap)
    _, want_d = _assert_closed(weights, ctx, actions, 'warp', tap, s3.CLOSED_T)
    if context == 'inside':          # one-hot all the way: the distribution IS the pixel trajectory
        pixels = s3.shifted_pixels(pix, tap, s3.CLOSED_T, s3.CLOSED_H, s3.CLOSED_W)
        for t in range(s3.CLOSED_T):
            for p in range(pixels.shape[1]):
                assert want_d[t, pixels[t, p, 0], pixels[t, p, 1], p] == 1.0
        # the other kernels' tap would put the pixel elsewhere: a swapped kernel index is visible
        assert s3.other_tap(tap) != tap


def test_float64_oracle_agrees_with_the_box_mean_when_every_tap_is_dead():
    weights, ctx, actions, _, _ = s3.closed_case(2, 'corner', dead=True, T=1)
    _assert_closed(weights, ctx, actions, 'dead', None, 1)


def test_float64_oracle_agrees_with_the_closed_forms_of_both_views():
    weights, ctx, actions, _ = s3.two_view_case()
    for v, slot in enumerate((s3.SLOT_PREV, s3.SLOT_FIRST)):
        cv = s3.view_of(ctx, v)
        _assert_closed(weights[v], cv, actions, s3.closed_kind(slot), None, 2)
