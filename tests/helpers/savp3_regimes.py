"""Weight regimes of the published SAVP generator (arch 'savp3') away from the Glorot initialisation, and networks whose
rollout has a closed form (test infrastructure; the savp3 companion of weight_regimes.py).

Every other device test of arch 'savp3' runs ``CdnaWeights.random(..., bias_scale=0.05, ln_jitter=0.1)``: instance-norm
variances of 0.1 (1e5 times the epsilon), conditioning tables that carry a few percent of a layer, a flat mask softmax.
The builders here are plain NumPy on ``CdnaWeights.tensors`` (names: ``oracle/savp3_predictor.expected_shapes``):

* ``weight_regimes.raw_scaled``  power-of-two factors on the convs an instance norm follows; scaled DOWN the variance falls to
                                 or below the epsilon, which becomes a first-order term of the output;
* ``cond_scaled``                the conditioning rows of every conv and gate conv times a power of two: the border-class
                                 tables carry the layer;
* ``gate_offset``                gate-norm offsets from a level set (saturated gates);
* ``gain_scaled`` / ``conv_bias_offset`` / ``masks_w_scaled``   regimes in which the float32 oracle itself drifts from float64;
* ``slot_network``               one of the seven compositing slots at +100 (single-tap or dead CDNA kernels, a constant
                                 scratch image): ``closed_form`` gives frames and distributions in NumPy, sharing no code
                                 with the oracle.

``tests/test_savp3_regimes.py`` proves the CPU-side conditions of ``CASES``; ``tests/test_gpu_savp3_magnitudes.py`` runs them on
the device.
"""
import re
from collections import OrderedDict

import numpy as np

from oracle import pixel_cost
from tests.helpers.weight_regimes import _clone, raw_layer_names, raw_scaled
from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config, CdnaWeights

ADIM, ZDIM = 12, 8
FINAL_WEIGHT = 10.
SLOT_PREV, SLOT_FIRST, SLOT_SCRATCH = 4, 5, 6
SCRATCH_BIAS = (100., -100., 0.)
CLOSED_FORM_ORACLE_BOUND = 1e-10        # float64 oracle vs closed form, frames and distributions / plane max


# ---------------------------------------------------------------------------------------------------- networks
def base_weights(H, W, nd, T, spec=0, seed=3):
    cfg = Savp3Config(height=H, width=W, adim=ADIM, ndesig=nd, sequence_length=T + 2, zdim=ZDIM, layer_spec=spec)
    return CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)


def _power_of_two(f):
    f = float(f)
    if f <= 0 or np.frexp(f)[0] != 0.5:
        raise ValueError('factor %r is not a power of two' % f)
    return np.float32(f)


def cond_scaled(weights, factor):
    """The conditioning rows times a power of two: the last ``ncond`` input channels of every ``h{i}c/w`` ([x | v]), the
    input channels ``C .. C + ncond`` of every ``h{i}l/w`` ([x | v | h])."""
    out, f, nc = _clone(weights), _power_of_two(factor), weights.cfg.ncond
    for name, w in out.tensors.items():
        if re.match(r'h\d+c/w$', name):
            w[:, :, -nc:, :] *= f
        elif re.match(r'h\d+l/w$', name):
            C = w.shape[3] // 4
            assert w.shape[2] == 2 * C + nc
            w[:, :, C:C + nc, :] *= f
    return out


def gate_offset(weights, levels, seed):
    """``h{i}lg/b`` += a per-channel draw from ``levels``."""
    out, rs = _clone(weights), np.random.RandomState(seed)
    lv = np.asarray(levels, dtype=np.float32)
    for name, b in out.tensors.items():
        if re.match(r'h\d+lg/b$', name):
            b += lv[rs.randint(0, len(lv), b.shape)]
    return out


def gain_scaled(weights, name, factor):
    out = _clone(weights)
    out.tensors[name + '/g'] *= np.float32(factor)
    return out


def conv_bias_offset(weights, value):
    """Every conv bias in front of an instance norm (``h{i}c/b``, ``hm/b``, ``hs/b``) + ``value``: the norm removes it, the
    float32 arithmetic pays ``|mean| / sigma`` in bits."""
    out = _clone(weights)
    for name, b in out.tensors.items():
        if re.match(r'(h\d+c|hm|hs)/b$', name):
            b += np.float32(value)
    return out


def masks_w_scaled(weights, factor):
    out = _clone(weights)
    out.tensors['masks/w'] *= np.float32(factor)
    return out


def other_tap(tap):
    """The tap the kernels that are NOT under test get: the point mirror of ``tap`` (never equal to it: no tap used is the
    centre)."""
    return (4 - tap[0], 4 - tap[1])


def slot_network(weights, slot, tap=None, dead=False):
    """``masks/b`` + 100 on ``slot`` (0 .. 3 warps, 4 previous, 5 first, 6 scratch).  ``tap``: ``cdna/w = 0``, ``cdna/b`` = -50
    everywhere and +10 on ``tap`` of kernel ``slot`` and on ``other_tap(tap)`` of the other three;  ``dead``: ``cdna/w = 0``,
    ``cdna/b = -1`` (every tap relu(-1 - 1e-12) + 1e-12: a box mean);  slot 6: ``scratch/w = 0``, ``scratch/b = (100, -100, 0)``."""
    out = _clone(weights)
    out.tensors['masks/b'][slot] += np.float32(100.)
    if slot == SLOT_SCRATCH:
        out.tensors['scratch/w'][:] = 0.
        out.tensors['scratch/b'][:] = np.array(SCRATCH_BIAS, dtype=np.float32)
    if tap is not None or dead:
        out.tensors['cdna/w'][:] = 0.
        b = out.tensors['cdna/b'].reshape(25, 4)           # [tap][kernel] (a view)
        b[:] = -1. if dead else -50.
        if tap is not None:
            for k in range(4):
                ty, tx = tap if k == slot else other_tap(tap)
                b[5 * ty + tx, k] = 10.
    return out


# ---------------------------------------------------------------------------------------------------- closed forms
def sym_shift(img, tap):
    """One single-tap warp of ``img[H, W, C]``: ``out(y, x) = pad(y + ty, x + tx)`` of the symmetrically padded image."""
    H, W = img.shape[:2]
    pad = np.pad(img, ((2, 2), (2, 2), (0, 0)), mode='symmetric')
    return pad[tap[0]:tap[0] + H, tap[1]:tap[1] + W]


def box_mean(img):
    """All 25 taps equal: the 5 x 5 mean of the symmetrically padded image."""
    H, W = img.shape[:2]
    pad = np.pad(img, ((2, 2), (2, 2), (0, 0)), mode='symmetric')
    return sum(pad[ty:ty + H, tx:tx + W] for ty in range(5) for tx in range(5)) / 25.


def closed_form(ctx, kind, T, tap=None, view=0):
    """float64 frames [T, H, W, 3] and distributions [T, H, W, nd] of every candidate under a slot-saturated network.
    ``kind``: 'prev', 'first', 'scratch', 'warp' (with ``tap``), 'dead'."""
    frames = (ctx['context_frames'][:, view].astype(np.float32) / np.float32(255.)).astype(np.float64)
    distr = ctx['context_pixel_distributions'][:, view].astype(np.float64)
    f, d = frames[-1], distr[-1]
    out_f, out_d = [], []
    for _ in range(T):
        if kind == 'first':
            f, d = frames[-2], distr[-2]
        elif kind == 'scratch':
            f = np.broadcast_to(1. / (1. + np.exp(-np.array(SCRATCH_BIAS))), f.shape)
        elif kind == 'warp':
            f, d = sym_shift(f, tap), sym_shift(d, tap)
        elif kind == 'dead':
            f, d = box_mean(f), box_mean(d)
        elif kind != 'prev':
            raise ValueError(kind)
        d = d / d.sum(axis=(0, 1), keepdims=True)
        out_f.append(f); out_d.append(d)
    return np.stack(out_f), np.stack(out_d)


def shifted_pixels(pix, tap, T, H, W):
    """[T, nd, 2]: where a one-hot pixel sits after each step of the single-tap warp, as long as nothing reflects."""
    step = np.array([2 - tap[0], 2 - tap[1]])
    pixels = np.stack([np.asarray(pix) + (t + 1) * step for t in range(T)])
    assert (pixels >= 2).all() and (pixels[..., 0] < H - 2).all() and (pixels[..., 1] < W - 2).all(), 'a pixel reflects'
    return pixels


# ---------------------------------------------------------------------------------------------------- inputs
def make_inputs(cfg, M, T, seed, desig=None, goal=None, one_hot=False, ncam=1):
    """Context, actions, goal [ncam, nd, 2] and designated pixels [ncam, nd, 2].  Rows are drawn from [0, H), columns from
    [0, W); entries of ``desig`` / ``goal`` that are not None replace the draw of their task (in every view).  The second
    context distribution is mixed with a uniform plane unless ``one_hot``, so that the first and the previous one differ."""
    H, W, nd = cfg.height, cfg.width, cfg.ndesig
    rs = np.random.RandomState(seed)
    pix = np.stack([rs.randint(0, H, (ncam, nd)), rs.randint(0, W, (ncam, nd))], axis=-1)
    g = np.stack([rs.randint(-2, H + 2, (ncam, nd)), rs.randint(-2, W + 2, (ncam, nd))], axis=-1)
    for src, dst in ((desig, pix), (goal, g)):
        for p, v in enumerate(src or ()):
            if v is not None:
                dst[:, p] = v
    d = pixel_cost.one_hot_distrib(pix, 2, ncam, H, W, nd)
    if not one_hot:
        d[1] = 0.5 * d[1] + 0.5 / (H * W)
    a_env = ADIM - ZDIM
    ctx = {'context_frames': rs.randint(0, 256, (3, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': np.concatenate([rs.normal(0, 0.05, (2, a_env)), np.zeros((2, ZDIM))], axis=1),
           'context_states': rs.normal(0, 0.1, (3, 5)),
           'context_pixel_distributions': d}
    actions = np.concatenate([rs.normal(0, 0.1, (M, T, a_env)), rs.normal(0, 1.0, (M, T, ZDIM))], axis=2)
    return ctx, actions, g, pix


def oracle_for(weights, dtype):
    from oracle.savp3_predictor import OracleSavp3
    return OracleSavp3(weights, dtype)


def rollout(oracle, ctx, actions):
    return oracle.rollout(ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'],
                          ctx['context_states'], actions)


def view_of(ctx, v):
    return dict(ctx, context_frames=ctx['context_frames'][:, v:v + 1],
                context_pixel_distributions=ctx['context_pixel_distributions'][:, v:v + 1])


# ---------------------------------------------------------------------------------------------------- shared cases
# Shapes: 32 x 32 two-scale table; 40 x 56 the heads' 8 x 16 tiles hang over both edges, width no multiple of 16; 64 x 64
# three-scale table; 64 x 64 / 64 x 80 with layer_spec 128: deepest maps 4 x 4 / 4 x 5 (no interior border class on one or both
# axes); 32 x 40 with layer_spec 64: deepest map 4 x 5.
# 'well' cases: the float32 oracle stays within a quarter of the device tolerances of the float64 oracle (asserted on the
# CPU), the device is compared with the float32 oracle.  'ill' cases: the float32 oracle drifts (up to 1e-4), the device is
# held to 3 x that distance only.  M = parity samples; the 'bits' cases are rolled with 23.
DOWN10, DOWN14, UP10 = 2. ** -10, 2. ** -14, 2. ** 10
CORNERS = lambda H, W: [(0, 0), (H - 1, W - 1), (0, W - 1)]        # noqa: E731

CASES = OrderedDict([
    # ---- scaled down: one layer at a time
    ('down10-h0c-32',        dict(H=32, W=32, nd=1, kind='well', raw={'h0c': DOWN10}, desig=[(0, 0)], goal=[(-2, 33)])),
    ('down14-h1l-32',        dict(H=32, W=32, nd=1, kind='well', raw={'h1l': DOWN14}, desig=[(31, 31)])),
    ('down14-hm-64',         dict(H=64, W=64, nd=1, kind='well', raw={'hm': DOWN14}, desig=[(0, 63)])),
    ('down10-h3c-64',        dict(H=64, W=64, nd=2, kind='well', raw={'h3c': DOWN10})),
    # ---- scaled down: every layer
    ('down10-all-32',        dict(H=32, W=32, nd=2, kind='well', raw={'all': DOWN10}, desig=[(31, 31), None], bits=True)),
    ('down14-all-40x56',     dict(H=40, W=56, nd=4, kind='well', raw={'all': DOWN14}, desig=CORNERS(40, 56) + [None],
                                  goal=[(45, 3), None, None, (-2, -2)])),
    ('down14-all-64',        dict(H=64, W=64, nd=1, kind='well', raw={'all': DOWN14})),
    # ---- scaled up
    ('up10-all-32',          dict(H=32, W=32, nd=1, kind='well', raw={'all': UP10})),
    ('up10-h2l-64',          dict(H=64, W=64, nd=1, kind='well', raw={'h2l': UP10, 'h4c': UP10})),
    # ---- conditioning x 32: the border-class tables carry the layers
    ('cond32-64-spec128',    dict(H=64, W=64, nd=1, spec=128, kind='well', cond=32., desig=[(0, 0)], bits=True)),
    ('cond32-64x80-spec128', dict(H=64, W=80, nd=2, spec=128, kind='well', cond=32., desig=[(63, 79), (0, 79)])),
    ('cond32-32x40-spec64',  dict(H=32, W=40, nd=1, spec=64, kind='well', cond=32.)),
    ('cond32-40x56',         dict(H=40, W=56, nd=1, kind='well', cond=32., desig=[(39, 55)], goal=[(20, 60)])),
    # ---- forced tables on their own (Glorot; 64 x 80 / layer_spec 128 with a random pixel puts the float32 oracle at 1.1e-5 of a
    # flat plane from float64 - past the quarter tolerance - and is run with the conditioning x 32 only)
    ('glorot-64-spec128',    dict(H=64, W=64, nd=1, spec=128, kind='well', desig=[(63, 0)])),
    ('glorot-32x40-spec64',  dict(H=32, W=40, nd=1, spec=64, kind='well', desig=[(0, 39)])),
    # ---- gates
    ('gate4-32',             dict(H=32, W=32, nd=1, kind='well', gate=(-4., 0., 4.))),
    ('gate4-40x56',          dict(H=40, W=56, nd=2, kind='well', gate=(-4., 0., 4.), desig=[(0, 55), None])),
    # ---- every CDNA tap dead, no slot favoured
    ('dead-taps-32',         dict(H=32, W=32, nd=1, kind='well', dead=True)),
    # ---- the float32 oracle itself drifts
    ('gain8-h1lg-32',        dict(H=32, W=32, nd=1, kind='ill', gain=('h1lg', 8.))),
    ('gain8-h1lc-32',        dict(H=32, W=32, nd=1, kind='ill', gain=('h1lc', 8.))),
    ('gain8-hmn-40x56',      dict(H=40, W=56, nd=1, kind='ill', gain=('hmn', 8.))),
    ('bias8-32',             dict(H=32, W=32, nd=1, kind='ill', bias=8.)),
    ('bias8-40x56',          dict(H=40, W=56, nd=2, kind='ill', bias=8.)),
    # (+ 64 puts the float32 oracle at 6.4e-5 / 1.02e-4 from float64 even at one step: past the cap of 1e-4; + 32 is kept)
    ('bias32-32-1step',      dict(H=32, W=32, nd=1, T=1, kind='ill', bias=32.)),
    ('gate8-32-1step',       dict(H=32, W=32, nd=1, T=1, kind='ill', gate=(-8., 0., 8.))),
    ('masksw8-40x56',        dict(H=40, W=56, nd=1, kind='ill', masks_w=8.)),
])
WELL = [n for n, c in CASES.items() if c['kind'] == 'well']
ILL = [n for n, c in CASES.items() if c['kind'] == 'ill']
BITS = [n for n, c in CASES.items() if c.get('bits')]
SCALED_DOWN = [n for n, c in CASES.items() if any(f < 1 for f in c.get('raw', {}).values())]
FORCED_TABLES = [(64, 64, 128), (64, 80, 128), (32, 40, 64)]
PARITY_M, BITS_M = 3, 23


def _seed(name):
    return sum(ord(c) for c in name)


def case(name, M=PARITY_M, unscaled=False):
    """-> weights, ctx, actions [M], goal.  ``unscaled``: the same case without its raw factors (its Glorot twin)."""
    c = CASES[name]
    T = c.get('T', 2)
    w = base_weights(c['H'], c['W'], c['nd'], T, c.get('spec', 0))
    if 'raw' in c and not unscaled:
        raw = c['raw']
        w = raw_scaled(w, {n: raw['all'] for n in raw_layer_names(w)} if 'all' in raw else raw)
    if 'cond' in c:
        w = cond_scaled(w, c['cond'])
    if 'gate' in c:
        w = gate_offset(w, c['gate'], _seed(name))
    if c.get('dead'):
        w.tensors['cdna/w'][:] = 0.
        w.tensors['cdna/b'][:] = -1.
    if 'gain' in c:
        w = gain_scaled(w, *c['gain'])
    if 'bias' in c:
        w = conv_bias_offset(w, c['bias'])
    if 'masks_w' in c:
        w = masks_w_scaled(w, c['masks_w'])
    ctx, actions, goal, _ = make_inputs(w.cfg, max(M, BITS_M), T, _seed(name), c.get('desig'), c.get('goal'))
    return w, ctx, actions[:M], goal


# Closed-form cases: 40 x 56, 3 steps (dead taps: 1 step).  'inside': the pixels stay 2 pixels inside the image for 3 steps of
# either tap, one-hot context distributions (scores from the pixel trajectory);  'corner': a pixel starts in a corner, the
# closed form is the NumPy symmetric pad.
CLOSED_H, CLOSED_W, CLOSED_T, CLOSED_M = 40, 56, 3, 3
SHIFT_TAPS = ((0, 3), (4, 1))
CLOSED_CONTEXTS = OrderedDict([
    ('inside', dict(desig=[(20, 30), (12, 44)], goal=[(50, 70), (-2, 3)], one_hot=True)),
    ('corner', dict(desig=[(0, 0), (39, 55)], goal=[(0, 55), (20, 20)], one_hot=False)),
])
# under a single-tap warp the content moves by (2 - ty, 2 - tx): the corner it moves AWAY from, where the symmetric padding
# doubles the peak (from any other corner the peak leaves the image and the plane that is left is flat)
WARP_CORNERS = {(0, 3): [(0, 55), (1, 55)], (4, 1): [(39, 0), (38, 0)]}


def closed_case(slot, context='inside', tap=None, dead=False, T=CLOSED_T):
    """-> weights, ctx, actions, goal, pix [nd, 2]."""
    base = base_weights(CLOSED_H, CLOSED_W, 2, T)
    weights = slot_network(base, slot, tap, dead)
    c = CLOSED_CONTEXTS[context]
    desig = WARP_CORNERS[tap] if context == 'corner' and tap is not None else c['desig']
    ctx, actions, goal, pix = make_inputs(weights.cfg, CLOSED_M, T, 17 + len(context), desig, c['goal'], c['one_hot'])
    return weights, ctx, actions, goal, pix[0]


def closed_kind(slot, dead=False):
    return 'dead' if dead else 'warp' if slot < 4 else {SLOT_PREV: 'prev', SLOT_FIRST: 'first', SLOT_SCRATCH: 'scratch'}[slot]


def two_view_case(slots=(SLOT_PREV, SLOT_FIRST), T=2):
    """ncam = 2, a different saturated slot per view -> [weights per view], ctx, actions, goal."""
    weights = [slot_network(base_weights(CLOSED_H, CLOSED_W, 1, T, seed=3 + v), s) for v, s in enumerate(slots)]
    ctx, actions, goal, _ = make_inputs(weights[0].cfg, CLOSED_M, T, 29, ncam=2)
    return weights, ctx, actions, goal
