"""Weight regimes away from the Glorot initialisation, their CPU-side conditions and closed forms (test infrastructure).

Every GPU test of the LayerNorm predictors (arch 'cdna', 'savp', 'savp2') used to run ``CdnaWeights.random(..., bias_scale=0.05,
ln_jitter=0.1)``: raw pre-LayerNorm outputs below 3, gate pre-activations below 5, a nearly flat mask softmax.  This module
builds networks at the magnitudes of a trained checkpoint in ways the CPU oracle stays well conditioned under:

* ``raw_scaled``      power-of-two factors on the layers a LayerNorm follows directly (the scale cancels in the oracle, the
                      device's integer statistics see values beyond 128);
* ``bias_saturated``  per-channel biases that saturate gates, heads and CDNA kernels (a saturated unit is a constant);
* ``copy_network`` / ``shift_network``  two networks whose rollout has a closed form, independent of any oracle.

It also restates the device's exact LayerNorm statistics (``stat_q``, ``stat_q2``, ``StatSumD``, ``ln_from_totals`` of
``csrc/vf_conv_mfma.h``) in Python integers, and installs a recording probe on an oracle instance without editing it.
``tests/test_weight_regimes.py`` proves the conditions on the CPU; ``tests/test_gpu_magnitudes.py`` runs the same cases
(``RAW_CASES``, ``SATURATED_CASES``, ``CLOSED_CASES``) on the device.  Plain NumPy; torch only where an oracle is built or probed.
"""
import contextlib
import math
import re
from collections import OrderedDict

import numpy as np

from oracle import pixel_cost
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig, Savp2Config

CONFIGS = {'cdna': CdnaConfig, 'savp': SavpConfig, 'savp2': Savp2Config}

# raw layer -> the LayerNorm that normalises it (the layers whose statistics come from conv_epilogue<EPI_*RAW_STATS>, the fused
# top and conv_first_tile; the other LayerNorms follow a conv-LSTM's h = tanh(c) * sigmoid(o), bounded by 1)
RAW_LAYERS = {'cdna': OrderedDict([('enc0', 'ln1'), ('convt3', 'ln9')]),
              'savp': OrderedDict([('enc00', 'lna'), ('enc0', 'ln1'), ('convt3', 'ln9'), ('convt4', 'lnb')])}
RAW_LAYERS['savp2'] = RAW_LAYERS['savp']
FAST_PATH_LIMIT = 128.          # |v| below which a wave adds its statistics as float64 (vf_fused_top.h, vf_conv_first.h)
LN_EPS32 = float(np.float32(1e-12))
TESTED_FILL = 0.25              # sum v^2 / 2^31 up to which the statistics are tested
CLOSED_FORM_ORACLE_BOUND = 1e-10    # float64 oracle vs closed form on frames (asserted in tests/test_weight_regimes.py)


# ---------------------------------------------------------------------------------------------------- networks
def _clone(weights):
    return CdnaWeights(weights.cfg, OrderedDict((k, v.copy()) for k, v in weights.tensors.items()))


def raw_layer_names(weights):
    """The layers ``raw_scaled`` accepts: those a normalisation follows directly.  arch 'savp3' normalises every conv
    (``h{i}c``), every conv-LSTM gate conv (``h{i}l``, no bias) and the heads' hidden layers (``hm``, ``hs``) per instance."""
    if weights.cfg.arch == 'savp3':
        return [k[:-2] for k in weights.tensors if re.match(r'(h\d+[cl]|hm|hs)/w$', k)]
    return list(RAW_LAYERS[weights.cfg.arch])


def raw_scaled(weights, factors):
    """``w`` and ``b`` of the named raw layers times a power of two (exact in float32, so the layer's output is the unscaled
    one times the factor, bit for bit, and the normalisation behind it cancels it up to its epsilon)."""
    out = _clone(weights)
    raw = raw_layer_names(weights)
    for name, f in factors.items():
        if name not in raw:
            raise ValueError('%s is not a raw-statistic layer of arch %s' % (name, weights.cfg.arch))
        m, _ = math.frexp(float(f))
        if f <= 0 or m != 0.5:
            raise ValueError('factor %r of %s is not a power of two' % (f, name))
        gate_conv = weights.cfg.arch == 'savp3' and re.match(r'h\d+l$', name)       # (the only raw layers without a bias)
        for kind in ('/w',) if gate_conv else ('/w', '/b'):
            out.tensors[name + kind] *= np.float32(f)
    return out


def _prev_channel(arch):
    """Mask channel that multiplies the previous frame."""
    return 4 if arch == 'savp2' else 0


def _warp0_channel(arch):
    """Mask channel the compositing pairs with CDNA kernel 0."""
    return {'cdna': 2, 'savp': 3, 'savp2': 0}[arch]


def _single_tap_kernels(tensors, taps):
    """cdna/b: -50 everywhere, +10 on ``taps[k] = (ty, tx)`` of kernel k: relu(x - 1e-12) + 1e-12 leaves 24 taps at 1e-12."""
    b = tensors['cdna/b'].reshape(25, -1)
    for k, (ty, tx) in taps.items():
        b[:, k] = -50.
        b[5 * ty + tx, k] = 10.


def bias_saturated(weights, seed, mask_channel=None, mask_bias=0., rgb=True, kernels=True):
    """Saturation through biases: every conv-LSTM bias gets a per-channel offset from {0, +-8, +-20, +-100}, the scratch head
    (100, -100, 0), one mask channel ``mask_bias``, every CDNA kernel one live tap."""
    out = _clone(weights)
    rs = np.random.RandomState(seed)
    levels = np.array([0., 8., -8., 20., -20., 100., -100.], dtype=np.float32)
    for k in range(1, 8):
        b = out.tensors['lstm%d/b' % k]
        b += levels[rs.randint(0, len(levels), b.shape)]
    if rgb:
        out.tensors['rgb/b'] += np.array([100., -100., 0.], dtype=np.float32)
    if mask_channel is not None:
        out.tensors['masks/b'][mask_channel] += np.float32(mask_bias)
    if kernels:
        nk = out.tensors['cdna/b'].size // 25
        _single_tap_kernels(out.tensors, {k: (int(rs.randint(0, 5)), int(rs.randint(0, 5))) for k in range(nk)})
    return out


def copy_network(weights):
    """masks/b += 100 on the previous-frame channel: every predicted frame is the last context frame."""
    out = _clone(weights)
    out.tensors['masks/b'][_prev_channel(weights.cfg.arch)] += np.float32(100.)
    return out


def shift_network(weights, tap):
    """masks/b += 100 on the layer of CDNA kernel 0, kernel 0 = the single tap ``(ty, tx)``:
    ``next(y, x) = prev(y + ty - 2, x + tx - 2)``, zero outside the image."""
    out = _clone(weights)
    out.tensors['masks/b'][_warp0_channel(weights.cfg.arch)] += np.float32(100.)
    _single_tap_kernels(out.tensors, {0: tap})
    return out


def shift_image(img, tap):
    """NumPy closed form of one step of ``shift_network`` on ``img[H, W, ...]``."""
    dy, dx = 2 - tap[0], 2 - tap[1]             # content moves by (dy, dx)
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = img[ys, xs]
    return out


def closed_form_scores(pixels, goal, finalweight):
    """``pixels[T, nd, 2]``: where each task's pixel is at every predicted step -> (score, per_task[nd])."""
    T = pixels.shape[0]
    w = np.ones(T); w[-1] = finalweight
    dist = np.sqrt(((pixels - np.asarray(goal, dtype=np.float64).reshape(1, -1, 2)) ** 2).sum(-1))    # [T, nd]
    per_task = (dist * w[:, None]).sum(0) / w.sum()
    return per_task.mean(), per_task


# ---------------------------------------------------------------------------------------------------- range of the statistics
def stat_fill(raw):
    """sum v^2 / 2^31 per sample of ``raw[B, ...]``: the share of the int64 total of trunc(v^2 2^32) in use (must stay < 1)."""
    v = np.asarray(raw, dtype=np.float64)
    return (v.reshape(v.shape[0], -1) ** 2).sum(1) / float(1 << 31)


def stat_rms_limit(n):
    """Largest rms a layer of ``n`` elements per sample may have before the int64 total of its squares wraps."""
    return math.sqrt(float(1 << 31) / n)


# ---------------------------------------------------------------------------------------------------- integer restatement
def _trunc_scaled(num, den):
    """trunc(num / den * 2^32) for integers, den > 0."""
    q = (abs(num) << 32) // den
    return -q if num < 0 else q


def stat_q(v):
    """trunc(v * 2^32) of the float32 ``v``, in Python integers."""
    num, den = float(np.float32(v)).as_integer_ratio()
    return _trunc_scaled(num, den)


def stat_q2(v):
    """trunc(v^2 * 2^32) of the float32 ``v``, in Python integers."""
    num, den = float(np.float32(v)).as_integer_ratio()
    return _trunc_scaled(num * num, den * den)


def stat_totals(values):
    """Per-value path of the device: integer totals (sum, sum of squares) of float32 values."""
    flat = np.asarray(values, dtype=np.float32).ravel()
    return sum(stat_q(v) for v in flat), sum(stat_q2(v) for v in flat)


def stat_sum_d(values):
    """``StatSumD``: the same integers added one after the other as float64, converted once."""
    s = q = 0.0
    for v in np.asarray(values, dtype=np.float32).ravel():
        d = float(v)
        s += float(math.trunc(d * 4294967296.0))
        q += float(math.trunc(d * d * 4294967296.0))
    return int(s), int(q)


def stat_totals_fast(raw):
    """Integer totals of a whole float32 tensor (vectorised: object arrays of Python integers): the same numbers as
    ``stat_totals``, for tensors of 10^5 elements."""
    d = np.asarray(raw, dtype=np.float32).astype(np.float64).ravel()
    # d * 2^32 and d * d * 2^32 are exact in float64 (24- and 48-bit significands); the truncated values need up to 63 bits
    qs = np.trunc(d * 4294967296.0)
    q2 = np.trunc(d * d * 4294967296.0)
    return int(sum(int(x) for x in qs)), int(sum(int(x) for x in q2))


def ln_from_totals(su, sq, n):
    """mean, rstd (float32) from the integer totals of ``n`` elements, in the device's float64 steps."""
    inv_n = float(np.float32(1.0 / n))
    m = float(su) * (1.0 / 4294967296.0) * inv_n
    var = float(sq) * (1.0 / 4294967296.0) * inv_n - m * m
    var = max(var, 0.0)
    return np.float32(m), np.float32(1.0 / math.sqrt(var + LN_EPS32))


# ---------------------------------------------------------------------------------------------------- oracle probe
class Probe(object):
    """What ``probe`` records of one rollout."""

    def __init__(self):
        self.raw = OrderedDict()        # LayerNorm name -> dict(fill, frac128, vmax, n, first)
        self.gate_n = self.gate_20 = self.gate_88 = 0
        self.gate_max = 0.
        self.mass = []                  # smallest pre-normalisation mass of the designated-pixel layers, per step

    def gate_fraction(self, level):
        return (self.gate_20 if level == 20 else self.gate_88) / float(max(self.gate_n, 1))


@contextlib.contextmanager
def probe(oracle):
    """Record, for one ``oracle.rollout``: the tensors entering ``_ln`` behind a raw layer, the gate pre-activations of every
    conv-LSTM, and the mass the designated-pixel distributions hold before they are renormalised.  Installed on the
    instance (``OracleCdna`` / ``OracleSavp`` / ``OracleSavp2``); the oracle classes are untouched."""
    import torch
    from torch.overrides import TorchFunctionMode

    rec = Probe()
    raw_lns = set(RAW_LAYERS[oracle.cfg.arch].values())
    ln, conv = oracle._ln, oracle._conv

    def ln_hook(x, name):
        if name in raw_lns:
            v = x.detach().numpy()
            e = rec.raw.setdefault(name, dict(fill=0., frac128=0., vmax=0., n=int(v[0].size), first=v.copy()))
            e['fill'] = max(e['fill'], float(stat_fill(v).max()))
            e['frac128'] = max(e['frac128'], float((np.abs(v) >= FAST_PATH_LIMIT).mean()))
            e['vmax'] = max(e['vmax'], float(np.abs(v).max()))
        return ln(x, name)

    def conv_hook(x, name, stride=1):
        y = conv(x, name, stride)
        if name.startswith('lstm'):
            z = y.detach().abs()
            rec.gate_n += z.numel()
            rec.gate_20 += int((z > 20).sum())
            rec.gate_88 += int((z > 88).sum())
            rec.gate_max = max(rec.gate_max, float(z.max()))
        return y

    class MassTap(TorchFunctionMode):
        # the one reduction over dim (2, 3) of a step is the mass the next distributions are divided by
        def __torch_function__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if func is torch.Tensor.sum and kwargs and kwargs.get('dim') == (2, 3):
                rec.mass.append(float(out.min()))
            return out

    oracle._ln, oracle._conv = ln_hook, conv_hook
    try:
        with MassTap():
            yield rec
    finally:
        del oracle._ln, oracle._conv


# ---------------------------------------------------------------------------------------------------- shared cases
def base_weights(arch, H, W, nd, T, seed=3, adim=None, decoder='survey'):
    kw = dict(decoder=decoder) if arch == 'cdna' and decoder != 'survey' else {}
    cfg = CONFIGS[arch](height=H, width=W, adim=adim or (4 if arch == 'cdna' else 6), ndesig=nd, sequence_length=T + 2, **kw)
    return CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)


def make_inputs(cfg, M, T, seed, desig=None, goal=None, margin=0, one_hot=False):
    """Context, actions and goal of a case.  Designated rows come from [margin, H - margin), columns from
    [margin, W - margin); entries of ``desig`` / ``goal`` that are not None replace the draw of their task.  The context
    distributions are one-hot (arch 'cdna', or ``one_hot``) or, for the first-frame skip to be visible, the second one mixed
    with a uniform plane (as tests/test_gpu_savp.py)."""
    H, W, nd, adim = cfg.height, cfg.width, cfg.ndesig, cfg.adim
    rs = np.random.RandomState(seed)
    pix = np.stack([rs.randint(margin, H - margin, nd), rs.randint(margin, W - margin, nd)], axis=1)[None]
    g = np.stack([rs.randint(-2, H + 2, nd), rs.randint(-2, W + 2, nd)], axis=1)[None]
    for src, dst in ((desig, pix), (goal, g)):
        for p, v in enumerate(src or ()):
            if v is not None:
                dst[0, p] = v
    d = pixel_cost.one_hot_distrib(pix, 2, 1, H, W, nd)
    if cfg.arch != 'cdna' and not one_hot:
        d[1] = 0.5 * d[1] + 0.5 / (H * W)
    ctx = {'context_frames': rs.randint(0, 256, (3, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (2, adim)),
           'context_states': rs.normal(0, 0.1, (3, 5)),
           'context_pixel_distributions': d}
    return ctx, rs.normal(0, 0.1, (M, T, adim)), g, pix


def oracle_for(weights, dtype):
    from oracle.cdna_predictor import OracleCdna
    from oracle.savp_predictor import OracleSavp, OracleSavp2
    return {'cdna': OracleCdna, 'savp': OracleSavp, 'savp2': OracleSavp2}[weights.cfg.arch](weights, dtype)


def rollout(oracle, ctx, actions):
    return oracle.rollout(ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'],
                          ctx['context_states'], actions)


# Raw-scaled cases.  'parity' cases are compared with the float32 oracle on the device (M = 5); 'bits' cases run the strategy
# sweep (M = 37).  The CPU conditions are proven on the first CPU_M candidates of the same inputs: the raw layers of the
# context steps do not depend on the candidate at all, those of the predicted steps only through the actions' small effect.
# Factors per case (unscaled, the largest |v| is 1.0 - 1.3 in enc0 / enc00, 1.8 - 2.0 in arch 1 / 2's enc0, 2.5 - 3.0 in convt3,
# 2.0 - 2.3 in convt4): every case keeps one raw layer entirely below 128 and puts another on both sides of it.  A factor
# that leaves a fraction of 1e-4 .. 2e-3 of a layer beyond 128 splits its WAVES between the two branches (x64 on a top
# layer, x128 on enc00); from a few percent on every wave of the layer takes the per-value branch.
CPU_M = 3
SEED_FILL = 4           # inputs with which x256 on the 32 x 32 top layer lands just below the tested fill (0.248; others reach 0.253)
H_, W_ = 48, 64
RAW_CASES = OrderedDict([
    ('cdna-32',        dict(arch='cdna', H=32, W=32, nd=1, T=3, M=5, kind='parity', desig=[(0, 0)], goal=[(-2, 33)],
                            factors={'enc0': 256., 'convt3': 32.})),
    ('cdna-48x64',     dict(arch='cdna', H=H_, W=W_, nd=2, T=2, M=5, kind='parity', desig=[(H_ - 1, W_ - 1), (20, 60)],
                            goal=[(10, 65), None], factors={'enc0': 64., 'convt3': 64.})),
    ('cdna-public-64', dict(arch='cdna', H=64, W=64, nd=1, T=2, M=5, kind='parity', decoder='public', desig=[(0, 63)],
                            factors={'enc0': 64., 'convt3': 64.})),
    ('savp-32',        dict(arch='savp', H=32, W=32, nd=1, T=3, M=5, kind='parity',
                            factors={'enc00': 128., 'enc0': 128., 'convt3': 64., 'convt4': 64.})),
    ('savp2-64',       dict(arch='savp2', H=64, W=64, nd=2, T=2, M=5, kind='parity', desig=[(63, 63), None],
                            factors={'enc00': 256., 'enc0': 32., 'convt3': 256., 'convt4': 64.})),
    ('cdna-32-bits',   dict(arch='cdna', H=32, W=32, nd=2, T=3, M=37, kind='bits', factors={'enc0': 64., 'convt3': 64.})),
    ('cdna-64-bits',   dict(arch='cdna', H=64, W=64, nd=1, T=3, M=37, kind='bits', factors={'enc0': 64., 'convt3': 64.})),
    ('savp-64-bits',   dict(arch='savp', H=64, W=64, nd=1, T=2, M=37, kind='bits',
                            factors={'enc00': 512., 'enc0': 64., 'convt3': 64., 'convt4': 64.})),
    # the top layer at the tested fill, values up to 740: every wave of it on the per-value branch, against the per-layer
    # launch (always per value)
    ('cdna-32-bits-fill', dict(arch='cdna', H=32, W=32, nd=1, T=2, M=37, kind='bits', seed=SEED_FILL,
                               factors={'enc0': 64., 'convt3': 256.})),
    # one channel of the top layer lifted by 6 before the scaling: its values lie around 384 and ANY 64 of them have squares
    # that add up beyond 2^53 (asserted in tests/test_weight_regimes.py) - the situation the limit of 128 exists for, a
    # float64 sum of the integers may round here.  (It rounds by one part in 2^53 of a total that becomes a float32 mean and
    # rstd: a library with the fast branch forced still gives the same OUTPUT bits in every case, this one included -
    # profiles/magnitude_regimes.txt, section 3.  What the cases do catch is a per-value branch that is wrong.)
    ('cdna-32-bits-lane', dict(arch='cdna', H=32, W=32, nd=1, T=2, M=37, kind='bits', offset=('convt3', 0, 6.),
                               factors={'enc0': 64., 'convt3': 64.})),
])
LANE_TERMS = 64                 # values a lane of the fused top adds up

# Bias-saturated cases.  Every CDNA kernel is a single tap, so a designated pixel moves up to 2 pixels per step: the
# pixels start 8 pixels inside the image and the mass cannot leave it within T + 1 steps.
SATURATED_CASES = OrderedDict([
    ('cdna-32-warp',      dict(arch='cdna', H=32, W=32, nd=1, T=3, M=5, mask_channel=2, mask_bias=100.)),
    ('cdna-48x64-starved', dict(arch='cdna', H=H_, W=W_, nd=2, T=2, M=5, mask_channel=1, mask_bias=12.)),
    ('savp-32',           dict(arch='savp', H=32, W=32, nd=1, T=3, M=5)),
    # no mask favoured: every layer of the compositing carries weight, so the frames see the gates (with mask 2 at +100 the
    # rollout is a shift network whatever the conv-LSTMs compute); the network of the bf16x6 case
    ('cdna-32',           dict(arch='cdna', H=32, W=32, nd=1, T=3, M=5)),
])

# Closed-form cases: start pixels that stay inside the image for T steps of either tap (a step moves a pixel by 2 - tap).
CLOSED_CASES = OrderedDict([
    ('cdna-48x64', dict(arch='cdna', H=H_, W=W_, nd=2, T=3, M=4, desig=[(20, 60), (6, 50)], goal=[(50, 70), (-2, 3)])),
    ('savp-32',    dict(arch='savp', H=32, W=32, nd=1, T=3, M=4, desig=[(12, 25)], goal=[(31, 0)])),
])
SHIFT_TAPS = ((0, 3), (4, 1))


def _seed(name):
    return sum(ord(c) for c in name)


def raw_case(name, M=None):
    c = RAW_CASES[name]
    base = base_weights(c['arch'], c['H'], c['W'], c['nd'], c['T'], decoder=c.get('decoder', 'survey'))
    if 'offset' in c:
        layer, channel, value = c['offset']
        base = _clone(base)
        base.tensors[layer + '/b'][channel] += np.float32(value)
    weights = raw_scaled(base, c['factors'])
    ctx, actions, goal, _ = make_inputs(weights.cfg, c['M'], c['T'], c.get('seed', _seed(name)), c.get('desig'), c.get('goal'))
    return weights, ctx, actions[:M or c['M']], goal


def saturated_case(name, M=None):
    c = SATURATED_CASES[name]
    base = base_weights(c['arch'], c['H'], c['W'], c['nd'], c['T'])
    weights = bias_saturated(base, _seed(name), c.get('mask_channel'), c.get('mask_bias', 0.))
    ctx, actions, goal, _ = make_inputs(weights.cfg, c['M'], c['T'], _seed(name), margin=8)
    return weights, ctx, actions[:M or c['M']], goal


def closed_case(name, network, tap=None, M=None):
    """-> weights, ctx, actions, goal, pixels[T, nd, 2] (where the closed form puts every designated pixel)."""
    c = CLOSED_CASES[name]
    base = base_weights(c['arch'], c['H'], c['W'], c['nd'], c['T'])
    weights = copy_network(base) if network == 'copy' else shift_network(base, tap)
    ctx, actions, goal, pix = make_inputs(weights.cfg, c['M'], c['T'], _seed(name), c['desig'], c['goal'], one_hot=True)
    step = np.array([0, 0]) if network == 'copy' else np.array([2 - tap[0], 2 - tap[1]])
    pixels = np.stack([pix[0] + (t + 1) * step for t in range(c['T'])])
    assert (pixels >= 0).all() and (pixels[..., 0] < c['H']).all() and (pixels[..., 1] < c['W']).all()
    return weights, ctx, actions[:M or c['M']], goal, pixels


def closed_form_frames(ctx, network, tap, T):
    """float64 [T, H, W, 3]: what every candidate's predicted frames are."""
    f = (ctx['context_frames'][-1, 0].astype(np.float32) / np.float32(255.)).astype(np.float64)
    out = []
    for _ in range(T):
        if network == 'shift':
            f = shift_image(f, tap)
        out.append(f)
    return np.stack(out)
