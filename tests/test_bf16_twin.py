"""The rounding twin of the plain-bf16 mode (tests/helpers/oracle_bf16.py) is itself pinned: its rounding is the integer-bit
round-to-nearest-even, and where rounding changes nothing the twin IS the oracle."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle.cdna_predictor import OracleCdna                            # noqa: E402
from tests.helpers.oracle_bf16 import OracleCdnaBf16, rne_bits, round_bf16  # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights   # noqa: E402


def _planted():
    ulp = np.float32(2.0 ** -23)
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.5 + 2.0 ** -9, 3 + 2.0 ** -6, 2.0 ** -20 * (1 + 2.0 ** -8)], np.float32)
    vals = []
    for t in ties:
        e = np.float32(np.spacing(t))
        vals += [t, t + e, t - e]
    vals = np.array(vals, np.float32)
    rs = np.random.RandomState(0)
    return np.concatenate([vals, -vals, [0.0, -0.0, 1.0, -1.0, ulp], rs.normal(0, 1, 4096).astype(np.float32),
                           rs.normal(0, 1e-6, 256).astype(np.float32)]).astype(np.float32)


def test_rounding_helper_is_integer_bit_rne():
    x = _planted()
    want = rne_bits(x)
    got = round_bf16(torch.from_numpy(x)).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # through float64 as well (the float64 twin's path)
    got64 = round_bf16(torch.from_numpy(x.astype(np.float64))).numpy()
    assert np.array_equal(got64.astype(np.float32).view(np.uint32), want.view(np.uint32))
    # the ties really go both ways: 1 + 2^-8 down to 1 (even), 1 + 3 * 2^-8 up to 1 + 2^-6 (even)
    assert rne_bits(np.float32(1 + 2.0 ** -8)) == np.float32(1.0)
    assert rne_bits(np.float32(1 + 3 * 2.0 ** -8)) == np.float32(1 + 2.0 ** -6)
    assert rne_bits(np.float32(1 + 2.0 ** -8) + np.float32(2.0 ** -23)) == np.float32(1 + 2.0 ** -7)
    assert np.array_equal(rne_bits(want).view(np.uint32), want.view(np.uint32))          # idempotent


def test_twin_is_the_oracle_on_bf16_representable_operands():
    """One ``_lstm`` call in float64 with weights and inputs that are multiples of 1/16 in [-1, 1] (bf16-representable; every
    product and sum exact): the twin and OracleCdna agree bit for bit."""
    cfg = CdnaConfig(height=32, width=32, ndesig=1, sequence_length=3, n_context=2)
    weights = CdnaWeights.random(cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(1)
    w = weights.tensors['lstm1/w']
    weights.tensors['lstm1/w'] = (rs.randint(-16, 17, w.shape) / 16.0).astype(w.dtype)
    x = torch.from_numpy(rs.randint(-16, 17, (2, 32, 16, 16)) / 16.0)
    h = torch.from_numpy(rs.randint(-16, 17, (2, 32, 16, 16)) / 16.0)
    c = torch.from_numpy(rs.normal(0, 1, (2, 32, 16, 16)))
    a = OracleCdna(weights, torch.float64)._lstm(x, (c, h), 'lstm1', 32)
    b = OracleCdnaBf16(weights, torch.float64)._lstm(x, (c, h), 'lstm1', 32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    # ... and it is NOT the oracle once an operand needs rounding
    x2 = x + 2.0 ** -12
    a2 = OracleCdna(weights, torch.float64)._lstm(x2, (c, h), 'lstm1', 32)
    b2 = OracleCdnaBf16(weights, torch.float64)._lstm(x2, (c, h), 'lstm1', 32)
    assert not torch.equal(a2[0], b2[0])
