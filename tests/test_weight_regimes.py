"""The CPU-side conditions tests/test_gpu_magnitudes.py rests on, proven on the oracles for the very inputs it runs
(tests/helpers/weight_regimes.py): a regime that drifts with a seed fails here, not on the device.

* the float64 fast path of the exact LayerNorm statistics (``StatSumD``) gives the per-value integers up to its limit;
* the raw-scaled networks put waves on both sides of that limit, stay within the tested share of the int64 total, and
  leave the float32 oracle where it was (the factors are powers of two: LayerNorm cancels them);
* the bias-saturated networks reach the ends of the gate math and stay well conditioned;
* the copy and shift networks have the closed forms the device is compared with.
"""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests.helpers import weight_regimes as wr          # noqa: E402

FRAME_TOL, DISTRIB_TOL = 1e-5, 2e-5                      # tests/test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def _run(kind, name):
    """float64 (probed) and float32 rollouts of a case, on its first CPU_M candidates."""
    weights, ctx, actions, _ = (wr.raw_case if kind == 'raw' else wr.saturated_case)(name, M=wr.CPU_M)
    o64 = wr.oracle_for(weights, torch.float64)
    with wr.probe(o64) as rec64:
        f64, d64, _ = wr.rollout(o64, ctx, actions)
    o32 = wr.oracle_for(weights, torch.float32)
    with wr.probe(o32) as rec32:
        f32, d32, _ = wr.rollout(o32, ctx, actions)
    err_f = float(np.abs(f32 - f64).max())
    err_d = float((np.abs(d32 - d64) / d64.max(axis=(3, 4), keepdims=True)).max())
    return weights, rec64, rec32, err_f, err_d


# ------------------------------------------------------------------------------------------------ integer statistics
def _f32_below(x):
    return np.nextafter(np.float32(x), np.float32(0))


@pytest.mark.parametrize('terms', [64, 32])      # a lane of the fused top / EPI_*RAW_STATS tile; conv_first's CO
def test_stat_sum_d_equals_the_integer_sum_up_to_the_fast_path_limit(terms):
    rs = np.random.RandomState(terms)
    edge = _f32_below(128.)
    sets = {'random': rs.uniform(-128, 128, terms).astype(np.float32),
            'all at the limit': np.full(terms, edge, dtype=np.float32),
            'alternating at the limit': np.where(np.arange(terms) % 2, edge, -edge).astype(np.float32),
            'around the limit': np.nextafter(np.float32(128.) - rs.uniform(0, 1e-3, terms).astype(np.float32),
                                             np.float32(0)) * np.where(rs.rand(terms) < .5, -1, 1).astype(np.float32),
            'tiny and zero': np.concatenate([np.zeros(terms // 2), rs.uniform(-1e-9, 1e-9, terms - terms // 2)])
                               .astype(np.float32)}
    for label, v in sets.items():
        assert np.abs(v).max() < wr.FAST_PATH_LIMIT
        assert wr.stat_sum_d(v) == wr.stat_totals(v), label
        assert wr.stat_totals_fast(v) == wr.stat_totals(v), label
    # at the limit a square is one float32 ulp below 2^14, the lane's 64 squares fill 2^52 of float64's 2^53
    for label in ('all at the limit', 'alternating at the limit'):
        sq = np.float32(sets[label][0]) * np.float32(sets[label][0])
        assert abs(float(sq) - 2. ** 14) <= float(np.spacing(np.float32(2. ** 14)))
    assert wr.stat_sum_d(sets['all at the limit'])[1] < 2 ** 53
    # truncation is towards zero on both paths
    assert wr.stat_q(np.float32(-1e-10)) == 0 and wr.stat_q(np.float32(-1.5)) == -(3 << 31)
    assert wr.stat_q2(np.float32(-3.)) == 9 << 32


def test_range_of_the_statistics():
    """Per element |v| < 46340 (v^2 2^32 < 2^63); per sample sum v^2 < 2^31, i.e. rms < sqrt(2^31 / n)."""
    assert wr.stat_q2(np.float32(46340.)) < 2 ** 63 <= wr.stat_q2(np.float32(46341.))
    assert wr.stat_rms_limit(2 ** 15) == 256. and wr.stat_rms_limit(2 ** 17) == 128. and wr.stat_rms_limit(2 ** 19) == 64.
    v = np.full((1, 2 ** 15), 255., dtype=np.float32)
    assert wr.stat_fill(v)[0] < 1. and wr.stat_totals_fast(v)[1] < 2 ** 63
    assert wr.stat_fill(np.full((1, 2 ** 15), 257., dtype=np.float32))[0] > 1.
    with pytest.raises(ValueError):
        wr.raw_scaled(wr.base_weights('cdna', 32, 32, 1, 2), {'enc0': 96.})
    with pytest.raises(ValueError):
        wr.raw_scaled(wr.base_weights('cdna', 32, 32, 1, 2), {'lstm1': 2.})


# ------------------------------------------------------------------------------------------------ raw-scaled networks
@pytest.mark.parametrize('name', list(wr.RAW_CASES))
def test_raw_scaled_case_mixes_the_branches_and_keeps_the_oracle(name):
    weights, rec64, rec32, err_f, err_d = _run('raw', name)
    arch = weights.cfg.arch
    assert list(rec32.raw) == list(wr.RAW_LAYERS[arch].values())
    for ln_name, e in rec32.raw.items():
        print('raw %-15s %-4s n=2^%-2d rms limit %5.0f  max|v| %6.1f  fraction >= 128 %.4f  fill %.4f'
              % (name, ln_name, round(math.log2(e['n'])), wr.stat_rms_limit(e['n']), e['vmax'], e['frac128'], e['fill']))
        assert e['fill'] <= wr.TESTED_FILL
    assert any(1e-4 < e['frac128'] < 0.5 for e in rec32.raw.values()), 'no raw layer with both branches in one sample'
    assert any(e['vmax'] < wr.FAST_PATH_LIMIT for e in rec32.raw.values()), 'no raw layer entirely on the fast path'
    print('raw %-15s float32 oracle vs float64: frames %.2e  distributions %.2e' % (name, err_f, err_d))
    assert err_f <= FRAME_TOL / 4 and err_d <= DISTRIB_TOL / 4
    # the integer statistics of the float32 oracle's raw tensors against float64 statistics of the same tensors: float32
    # rounding of the two results (2^-24 each) is all that may separate them - bound 2^-23
    for ln_name, e in rec32.raw.items():
        v = e['first'][0].astype(np.float32)
        mean, rstd = wr.ln_from_totals(*wr.stat_totals_fast(v), n=v.size)
        v64 = v.astype(np.float64)
        rms = math.sqrt((v64 ** 2).mean())
        assert abs(float(mean) - v64.mean()) <= 2. ** -23 * rms
        assert abs(float(rstd) * v64.std() - 1.) <= 2. ** -23


def test_lane_case_needs_the_per_value_branch():
    """'cdna-32-bits-lane': every value of the lifted channel is so large that the squares of any 64 of them - whatever lane
    they fall into - add up beyond 2^53, where a float64 sum of the integers trunc(v^2 2^32) is no longer exact."""
    weights, ctx, actions, _ = wr.raw_case('cdna-32-bits-lane', M=wr.CPU_M)
    layer, channel, _ = wr.RAW_CASES['cdna-32-bits-lane']['offset']
    o32 = wr.oracle_for(weights, torch.float32)
    with wr.probe(o32) as rec:
        wr.rollout(o32, ctx, actions)
    v = rec.raw[wr.RAW_LAYERS['cdna'][layer]]['first'][:, channel]
    smallest = float(np.abs(v).min())
    print('raw cdna-32-bits-lane  channel %d of %s: |v| in [%.1f, %.1f]' % (channel, layer, smallest, np.abs(v).max()))
    assert wr.LANE_TERMS * wr.stat_q2(np.float32(smallest)) > 2 ** 53
    exact = wr.stat_totals(v.ravel()[:wr.LANE_TERMS])
    assert wr.stat_sum_d(v.ravel()[:wr.LANE_TERMS])[0] == exact[0]          # the sum of v itself stays exact


def test_power_of_two_scaling_is_invisible_to_the_float64_oracle():
    name = 'cdna-32'
    c = wr.RAW_CASES[name]
    weights, ctx, actions, _ = wr.raw_case(name, M=wr.CPU_M)
    plain = wr.base_weights(c['arch'], c['H'], c['W'], c['nd'], c['T'])
    f_scaled = wr.rollout(wr.oracle_for(weights, torch.float64), ctx, actions)[0]
    f_plain = wr.rollout(wr.oracle_for(plain, torch.float64), ctx, actions)[0]
    assert np.abs(f_scaled - f_plain).max() <= 1e-10


# ------------------------------------------------------------------------------------------------ bias-saturated networks
@pytest.mark.parametrize('name', list(wr.SATURATED_CASES))
def test_bias_saturated_case_is_saturated_and_well_conditioned(name):
    weights, rec64, rec32, err_f, err_d = _run('saturated', name)
    print('saturated %-18s gates |z| > 20: %.3f  > 88: %.3f  max %.0f  smallest mass %.2e  float32 oracle vs float64: '
          'frames %.2e  distributions %.2e' % (name, rec64.gate_fraction(20), rec64.gate_fraction(88), rec64.gate_max,
                                                 min(rec64.mass), err_f, err_d))
    assert err_f <= FRAME_TOL / 4 and err_d <= DISTRIB_TOL / 4
    assert len(rec64.mass) == wr.SATURATED_CASES[name]['T'] + 1 and min(rec64.mass) >= 1e-7
    assert rec64.gate_fraction(20) >= 0.10
    assert rec64.gate_20 > rec64.gate_88 > 0            # __expf beyond overflow (88.7), and the range in between


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize('network,tap', [('copy', None)] + [('shift', t) for t in wr.SHIFT_TAPS])
@pytest.mark.parametrize('name', list(wr.CLOSED_CASES))
def test_closed_form_networks(name, network, tap):
    weights, ctx, actions, goal, pixels = wr.closed_case(name, network, tap, M=2)
    T = wr.CLOSED_CASES[name]['T']
    f64, d64, _ = wr.rollout(wr.oracle_for(weights, torch.float64), ctx, actions)
    want = wr.closed_form_frames(ctx, network, tap, T)
    err = float(np.abs(f64[:, :, 0] - want[None]).max())
    print('closed form %-10s %-5s %-6s float64 oracle vs closed form: frames %.2e' % (name, network, tap, err))
    assert err <= wr.CLOSED_FORM_ORACLE_BOUND
    for t in range(T):
        for p in range(pixels.shape[1]):
            plane = d64[:, t, 0, :, :, p]
            y, x = pixels[t, p]
            assert (plane.reshape(len(plane), -1).argmax(1) == y * plane.shape[2] + x).all()
            assert plane[:, y, x].min() >= 1 - 1e-9
    if name == 'cdna-48x64' and tap == (0, 3):          # the worked example: (20, 60) -> (22, 59) -> (24, 58) -> (26, 57)
        assert pixels[:, 0].tolist() == [[22, 59], [24, 58], [26, 57]]
