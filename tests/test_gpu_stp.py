"""GPU: the STP predictor (``StpConfig``) through the C ABI against the helper oracle of
``tests/helpers/oracle_stp.py``, against closed forms, and against itself over the three launch routes, batch splits and the
frames-only engine.

Bounds of the parity tests are those of ``test_gpu_parity.py::test_rollout_matches_oracle``: frames 1e-5, distributions 2e-5
of the plane maximum, states 1e-6, scores rtol 1e-5, device scores against the host cost of the device's distributions 2e-6,
planes sum to 1 within 2e-6.  Whether they may be used where a parameter error moves a gather is decided by the float32
helper's own distance to its float64 mode at the very inputs of each test, measured on the CPU
(``profiles/stp.txt`` section 1; ``tools/stp_bench.py --helper-distance``): see the two parity tests.
"""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                           # noqa: E402
from tests.helpers.oracle_stp import OracleStp, make_stp_predictor_class                   # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaWeights                    # noqa: E402
from visual_foresight_amd.video_prediction.stp_arch import StpConfig                       # noqa: E402

IDENT = np.float32([1, 0, 0, 0, 1, 0])


def _config(H, W, T, nd, n_context=2):
    return StpConfig(height=H, width=W, ndesig=nd, sequence_length=T + n_context, n_context=n_context)


def _predictor(H, W, T, nd, bs, seed=3, n_context=2, weights=None, **extra):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + n_context, n_context=n_context, transformation='stp', **extra)
    pred = HipVPredEvaluation('', hp)
    assert isinstance(pred.cfg, StpConfig) and pred.cfg.layer_spec == 4 and pred.cfg.num_masks == 10
    if weights is None:
        weights = stp_weights(_config(H, W, T, max(nd, 1), n_context), seed)
    pred.restore(weights)
    return pred, weights


STP_W_SCALE = 0.1       # of the Glorot draw of stp/w: the parameters leave the identity by about +-0.3 (profiles/stp.txt)


def stp_weights(cfg, seed):
    """Random weights of the full-parity tests: every tensor drawn, ``stp/w`` scaled by ``STP_W_SCALE``."""
    weights = CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)
    weights.tensors['stp/w'] *= np.float32(STP_W_SCALE)
    return weights


def _context(H, W, nd, rs, hist=3, desig=None):
    if desig is None:
        desig = np.stack([rs.randint(0, H, (1, nd)), rs.randint(0, W, (1, nd))], axis=-1)
    return {'context_frames': rs.randint(0, 256, (hist, 1, H, W, 3)).astype(np.uint8),
            'context_actions': rs.normal(0, 0.05, (hist - 1, 4)),
            'context_states': rs.normal(0, 0.1, (hist, 5)),
            'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, 2, 1, H, W, nd)}


# (H, W, n_context, T, M, nd).  The five tuples of the issue read in that order, and the same five tuples read in the order
# test_gpu_dna.py gives its own (H, W, T, M, nd, n_context) - which adds four designated pixels and one context frame.
PARITY_CASES = [(32, 32, 2, 5, 1, 2), (48, 64, 2, 5, 2, 2), (64, 64, 2, 3, 4, 2),
                (40, 56, 2, 4, 1, 2),          # a shape whose top cannot be fused: two phases
                (32, 32, 2, 4, 1, 1),
                (32, 32, 2, 2, 5, 1), (48, 64, 2, 2, 5, 2), (64, 64, 2, 2, 3, 4),
                (40, 56, 2, 2, 4, 1),          # two phases
                (32, 32, 1, 2, 4, 1)]          # one context frame


def fixed_transforms(H, W):
    """Nine transforms (normalised, identity included) for the head-out test: rotations, zooms 0.5 and 2, shears,
    translations of several pixels (a normalised translation t moves the sample point by ``t * (W - 1) / 2`` pixels), some
    sampling off-image."""
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    rot = lambda a, z=1.0: [z * np.cos(a), -z * np.sin(a), 0, z * np.sin(a), z * np.cos(a), 0]
    t = np.array([rot(0.3), rot(-1.1, 1.3), [0.5, 0, 0, 0, 0.5, 0], [2, 0, 0, 0, 2, 0], [1, 0.35, 0, 0, 1, 0],
                  [1, 0, 0, -0.5, 1, 0], [1, 0, 3.25 / sx, 0, 1, -2.5 / sy], [1, 0, -7.75 / sx, 0, 1, 6.0 / sy],
                  [0.8, 0.1, 0.9, -0.2, 1.1, -0.8]], np.float64)
    return t.astype(np.float32)


def parity_inputs(H, W, T, M, nd, nc, head_out):
    """Weights and inputs of one parity case (also used on the CPU to measure the helper against its float64 mode).
    ``head_out``: ``stp_fc/w = stp/w = 0`` and ``stp/b`` = nine fixed transforms minus the identity."""
    weights = stp_weights(_config(H, W, T, nd, nc), seed=3)
    if head_out:
        t = weights.tensors
        t['stp_fc/w'][:] = 0
        t['stp/w'][:] = 0
        t['stp/b'][:] = (fixed_transforms(H, W) - IDENT[None]).reshape(-1)
    rs = np.random.RandomState(H + W + T + M + nc)
    ctx = _context(H, W, nd, rs, hist=3 if nc == 2 else 1)
    if nc == 1:
        ctx['context_pixel_distributions'] = ctx['context_pixel_distributions'][:1]
        ctx['context_actions'] = np.zeros((0, 4))
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(-2, max(H, W) + 2, (1, nd, 2))          # goals may lie off-image
    return weights, ctx, actions, goal


def _oracle(weights, ctx, actions, dtype=torch.float32):
    return OracleStp(weights, dtype).rollout(ctx['context_frames'], ctx['context_actions'],
                                             ctx['context_pixel_distributions'], ctx['context_states'], actions)


# the bounds of test_gpu_parity.py::test_rollout_matches_oracle
CDNA_BOUNDS = dict(frames=1e-5, distrib=2e-5, states=1e-6, scores=1e-5)


def _check_parity(H, W, T, M, nd, nc, head_out, bounds, label):
    weights, ctx, actions, goal = parity_inputs(H, W, T, M, nd, nc, head_out)
    pred, _ = _predictor(H, W, T, nd, bs=M, n_context=nc, weights=weights)
    scores, per_task = pred.score(ctx, {'actions': actions}, goal, finalweight=10.)
    got = pred(ctx, {'actions': actions})
    f, d, s = _oracle(weights, ctx, actions)
    err_f = np.abs(got['predicted_frames'] - f).max()
    dmax = d.max(axis=(3, 4), keepdims=True)
    err_d = (np.abs(got['predicted_pixel_distributions'] - d) / dmax).max()
    err_s = np.abs(got['predicted_states'] - s).max()
    want, want_pt = pixel_cost.eval_pixel_cost(d, goal, 10.)
    err_c = np.abs(scores / want - 1).max()
    err_sum = np.abs(got['predicted_pixel_distributions'].sum(axis=(3, 4)) - 1.0).max()
    own, _ = pixel_cost.eval_pixel_cost(got['predicted_pixel_distributions'], goal, 10.)
    print('stp %s %dx%d nd %d nc %d: frames %.3g  distrib/planemax %.3g  states %.3g  scores rel %.3g  own cost rel %.3g  '
          '|sum - 1| %.3g' % (label, H, W, nd, nc, err_f, err_d, err_s, err_c, np.abs(scores / own - 1).max(), err_sum))
    assert err_f <= bounds['frames']
    assert err_d <= bounds['distrib']
    assert err_s <= bounds['states']
    np.testing.assert_allclose(scores, want, rtol=bounds['scores'])
    np.testing.assert_allclose(per_task, want_pt, rtol=bounds['scores'])
    np.testing.assert_allclose(scores, own, rtol=2e-6)
    assert err_sum <= 2e-6
    assert pred.device_status() == 0


@pytest.mark.parametrize('H,W,nc,T,M,nd', PARITY_CASES)
def test_compositing_matches_oracle_with_the_head_taken_out(H, W, nc, T, M, nd):
    """``stp_fc/w = stp/w = 0``: ``theta = stp/b + identity`` - nine different rotations, zooms (0.5 and 2), shears and
    translations of several pixels, some sampling off-image - with random mask and scratch heads.  The transforms do not
    depend on the first FC's summation order, so the bounds are the cdna bounds as they stand."""
    _check_parity(H, W, T, M, nd, nc, True, CDNA_BOUNDS, 'head out')


# Bounds of the full-parity test.  The first FC's summation order differs from the helper's (K-split MFMA GEMM against a
# matrix product) and a parameter error moves a gather, so the cdna bounds are not copied: HELPER_DISTANCE is the float32
# helper's distance to its float64 mode at these very inputs, measured on the CPU (profiles/stp.txt section 1, largest over
# the ten cases).  Per quantity: where that distance is at most a quarter of the cdna bound, the cdna bound; otherwise
# four times the measured distance (the ratio the DNA docstring holds itself to).  Never tuned from device output.
HELPER_DISTANCE = dict(frames=5.93e-6, distrib=2.10e-5, states=4.62e-8, scores=4.21e-7)


def full_parity_bounds():
    return {k: (CDNA_BOUNDS[k] if HELPER_DISTANCE[k] <= CDNA_BOUNDS[k] / 4 else 4 * HELPER_DISTANCE[k]) for k in CDNA_BOUNDS}


@pytest.mark.parametrize('H,W,nc,T,M,nd', PARITY_CASES)
def test_rollout_matches_oracle(H, W, nc, T, M, nd):
    """Full parity, every tensor random (``stp/w`` scaled by 0.1: the parameters leave the identity by 0.24 - 0.38).
    Measured helper distances (float32 against float64, largest of the ten cases): frames 5.93e-6 and distributions 2.10e-5
    of the plane maximum - both above a quarter of the cdna bounds (2.5e-6, 5e-6) - states 4.62e-8 and scores 4.21e-7 - both
    below (2.5e-7, 2.5e-6).  So the bounds are: frames 4 x 5.93e-6 = 2.372e-5, distributions 4 x 2.10e-5 = 8.4e-5 of the
    plane maximum, states 1e-6 and scores rtol 1e-5 (the cdna bounds)."""
    assert full_parity_bounds() == dict(frames=4 * 5.93e-6, distrib=4 * 2.10e-5, states=1e-6, scores=1e-5)
    _check_parity(H, W, T, M, nd, nc, False, full_parity_bounds(), 'full')


# ------------------------------------------------------------------------------------------ closed forms
def _affine_ref(img, theta):
    """The warp of the specification in NumPy float64: ``img [H, W, C]``, ``theta`` six normalised parameters (identity
    included) -> out[y, x] = clamped bilinear sample of img at (xs, ys)."""
    H, W = img.shape[:2]
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    cx, cy = (np.arange(W) - sx)[None, :], (np.arange(H) - sy)[:, None]
    t = [float(v) for v in theta]
    xs = np.clip(sx + t[0] * cx + t[1] * (sx / sy) * cy + t[2] * sx, 0, W - 1)
    ys = np.clip(sy + t[3] * (sy / sx) * cx + t[4] * cy + t[5] * sy, 0, H - 1)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (xs - x0)[..., None], (ys - y0)[..., None]
    img = img.astype(np.float64)
    top = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    bot = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    return top * (1 - fy) + bot * fy


def _closed_form_run(theta0, desig, H=32, W=32, T=2, M=3):
    """One designated pixel, zero ``stp_fc/w``, ``stp/w`` and ``masks/w``, ``masks/b`` = +40 on channel 2 (the mask of warp 0
    is 1.0 in fp32, the others 4e-18): every predicted frame is warp 0 of the frame before it, and ``stp/b`` gives warp 0 the
    transform ``theta0`` (the other eight any transform: their masks are 4e-18).  -> (last context frame [H, W, 3] float64,
    one-hot plane [H, W, 1], predicted frames [M, T, H, W, 3], predicted distributions [M, T, H, W], predictor)."""
    weights = CdnaWeights.random(_config(H, W, T, 1), seed=7, bias_scale=0.05, ln_jitter=0.1)
    t = weights.tensors
    t['stp_fc/w'][:] = 0
    t['stp/w'][:] = 0
    t['masks/w'][:] = 0
    t['masks/b'][:] = 0
    t['masks/b'][2] = 40.
    t['stp/b'][:] = np.random.RandomState(1).uniform(-0.5, 0.5, 54)
    t['stp/b'][:6] = np.asarray(theta0, np.float32) - IDENT
    pred, _ = _predictor(H, W, T, 1, bs=M, weights=weights)
    rs = np.random.RandomState(21)
    ctx = _context(H, W, 1, rs, desig=np.array([[desig]]))
    got = pred(ctx, {'actions': rs.normal(0, 0.1, (M, T, 4))})
    last = ctx['context_frames'][-1, 0].astype(np.float32) / np.float32(255.)
    onehot = np.zeros((H, W, 1))
    onehot[desig] = 1.
    return (last.astype(np.float64), onehot, got['predicted_frames'][:, :, 0],
            got['predicted_pixel_distributions'][:, :, 0, :, :, 0], pred)


def _check_closed_form(theta0, desig, label, H=32, W=32, T=2):
    """Every step against the float64 warp applied step after step; the designated pixel's plane likewise (renormalised)."""
    last, onehot, f, d, pred = _closed_form_run(theta0, desig, H=H, W=W, T=T)
    want_f, want_d, errs = last, onehot, []
    for s in range(T):
        want_f, want_d = _affine_ref(want_f, theta0), _affine_ref(want_d, theta0)
        want_d = want_d / want_d.sum()
        errs.append((np.abs(f[:, s] - want_f[None]).max(), np.abs(d[:, s] - want_d[None, :, :, 0]).max()))
    print('stp closed form %s: per step (frame err, distribution err) %s'
          % (label, ', '.join('(%.3g, %.3g)' % e for e in errs)))
    assert all(ef <= 1e-6 and ed <= 1e-6 for ef, ed in errs)            # (the tolerance of appflow's translation test)
    assert pred.device_status() == 0
    return last, onehot, f, d


def test_closed_form_identity_gives_the_previous_frame():
    last, onehot, f, d = _check_closed_form([1, 0, 0, 0, 1, 0], (15, 17), 'identity')
    assert np.abs(f - last[None, None]).max() <= 1e-6 and np.abs(d - onehot[None, None, :, :, 0]).max() <= 1e-6


def test_closed_form_shift_crosses_tile_edges_and_clamps_at_the_borders():
    """xs = x + 3, ys = y - 2 (``t2 = 3 / sx``, ``t5 = -2 / sy``): the edge-clamped shifted frame; the designated pixel
    (15, 17) moves to (17, 14), across both edges of the 16-pixel tiles."""
    H = W = 32
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    theta = [1, 0, 3 / sx, 0, 1, -2 / sy]
    last, onehot, f, d = _check_closed_form(theta, (15, 17), 'shift (+3, -2)')
    ys, xs = np.clip(np.arange(H) - 2, 0, H - 1), np.clip(np.arange(W) + 3, 0, W - 1)
    np.testing.assert_allclose(f[:, 0], np.broadcast_to(last[np.ix_(ys, xs)], f[:, 0].shape), rtol=0, atol=1e-6)
    assert (np.abs(d[:, 0, 17, 14] - 1) <= 1e-6).all() and (np.abs(d[:, 1, 19, 11] - 1) <= 1e-6).all()


def test_closed_form_flip_reads_the_far_corner_of_the_previous_step():
    """``theta = (-1, 0, 0, 0, -1, 0)`` flips both axes exactly: every tile reads the far corner of the frame the previous
    step composed (64 x 64: sixteen compositing tiles, T = 3 - steps 2 and 3 read device-made frames).  A tile that started
    before the far tile of the previous step was written would show here: the test of the whole-frame dependency."""
    last, onehot, f, d = _check_closed_form([-1, 0, 0, 0, -1, 0], (17, 40), 'flip', H=64, W=64, T=3)
    np.testing.assert_allclose(f[:, 0], np.broadcast_to(last[::-1, ::-1], f[:, 0].shape), rtol=0, atol=1e-6)
    np.testing.assert_allclose(f[:, 1], np.broadcast_to(last, f[:, 1].shape), rtol=0, atol=1e-6)
    np.testing.assert_allclose(f[:, 2], np.broadcast_to(last[::-1, ::-1], f[:, 2].shape), rtol=0, atol=1e-6)
    assert (np.abs(d[:, 0, 63 - 17, 63 - 40] - 1) <= 1e-6).all() and (np.abs(d[:, 1, 17, 40] - 1) <= 1e-6).all()


def test_closed_form_zoom_half_averages_neighbours():
    """Zoom 0.5 about the centre: ``xs = sx + (x - sx) / 2`` lies a quarter (x odd) or three quarters (x even) between two
    pixels, so every output pixel is the (1/4, 3/4) x (1/4, 3/4) average of four neighbours."""
    last, onehot, f, d = _check_closed_form([0.5, 0, 0, 0, 0.5, 0], (15, 17), 'zoom 0.5')
    y, x = 10, 13                       # ys = 15.5 + (10 - 15.5) / 2 = 12.75, xs = 15.5 + (13 - 15.5) / 2 = 14.25
    want = 0.25 * (0.75 * last[12, 14] + 0.25 * last[12, 15]) + 0.75 * (0.75 * last[13, 14] + 0.25 * last[13, 15])
    np.testing.assert_allclose(f[:, 0, y, x], np.broadcast_to(want, f[:, 0, y, x].shape), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------ routes, batches, frames-only
ROUTES = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1)]          # (persistent, fuse_top, xcd_queues)


@pytest.mark.parametrize('H,W,nd,M,T', [pytest.param(32, 32, 2, 9, 3, id='32-32-2-9'), pytest.param(64, 64, 4, 6, 3, id='64-64-4-6'),
                                        pytest.param(32, 32, 1, 3, 2, id='32-32-1-3-T2'), pytest.param(32, 32, 3, 3, 2, id='32-32-3-3-T2')])
def test_launch_routes_are_invisible_in_the_results(H, W, nd, M, T):
    """Fused top, two-phase persistent schedule and per-layer launches - the persistent ones with the XCD queues on and off
    - run the same per-pixel code on the same floats: the same bits for scores, frames, distributions and states, in a
    second call (cached context) and with every sequence moved to another slot of the batch.  The four cases are the four
    designated-pixel counts the kernels are instantiated for (the shapes of test_gpu_dna.py's test of this name)."""
    pred, _ = _predictor(H, W, T, nd, bs=M, seed=5)
    rs = np.random.RandomState(H + M)
    ctx = _context(H, W, nd, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, min(H, W), (1, nd, 2))
    perm = np.roll(np.arange(M), 1)
    outs = []
    for persistent, fuse, xcd in ROUTES:
        pred.set_persistent(persistent)
        pred.set_fuse_top(fuse)
        pred.set_xcd_queues(xcd)
        for rep in range(2):
            s, pt = pred.score(ctx, {'actions': actions}, goal)
            assert pred.device_status() == 0
            if rep:
                np.testing.assert_array_equal(s, s_first)
            s_first = s
        got = pred(ctx, {'actions': actions})
        sp, _ = pred.score(ctx, {'actions': actions[perm]}, goal)
        gp = pred(ctx, {'actions': actions[perm]})
        np.testing.assert_array_equal(sp, s[perm])
        np.testing.assert_array_equal(gp['predicted_frames'], got['predicted_frames'][perm])
        np.testing.assert_array_equal(gp['predicted_pixel_distributions'], got['predicted_pixel_distributions'][perm])
        np.testing.assert_array_equal(gp['predicted_states'], got['predicted_states'][perm])
        outs.append((s, pt, got['predicted_frames'], got['predicted_pixel_distributions'], got['predicted_states']))
        pred._ctx_key = None                    # upload the context again: the next route computes the shared units itself
    assert np.isfinite(outs[0][0]).all() and np.ptp(outs[0][0]) > 0
    assert np.abs(outs[0][2][0] - outs[0][2][1]).max() > 0                  # the actions matter (through the FC head too)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)
    assert pred.device_status() == 0


def test_large_batch_equals_two_calls_of_half():
    """130 samples at 32 x 32, T = 1: two row tiles of the first FC (128 + 2 rows) and 130 finish items, against the same
    sequences run in two calls of 65 (one row tile each): equal bits."""
    H = W = 32
    T, M, nd = 1, 130, 1
    pred, _ = _predictor(H, W, T, nd, bs=M, seed=9)
    rs = np.random.RandomState(130)
    ctx = _context(H, W, nd, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, H, (1, nd, 2))
    s_all, _ = pred.score(ctx, {'actions': actions}, goal)
    got = pred(ctx, {'actions': actions})
    assert pred.device_status() == 0
    assert np.isfinite(s_all).all() and np.ptp(s_all) > 0
    for lo in (0, 65):
        s_half, _ = pred.score(ctx, {'actions': actions[lo:lo + 65]}, goal)
        half = pred(ctx, {'actions': actions[lo:lo + 65]})
        assert pred.device_status() == 0
        np.testing.assert_array_equal(s_half, s_all[lo:lo + 65])
        for k in ('predicted_frames', 'predicted_pixel_distributions', 'predicted_states'):
            np.testing.assert_array_equal(half[k], got[k][lo:lo + 65])


@pytest.mark.parametrize('H,W,M,ncam', [(32, 32, 5, 1), (48, 64, 9, 1), (40, 56, 5, 1), (32, 32, 5, 2)])
def test_frames_only_engine_equals_the_one_pixel_engine(H, W, M, ncam):
    """The frames and states of a frames-only stp engine (``designated_pixel_count`` 0) are those of the engine with one
    designated pixel, bit for bit, on all three launch routes; (40, 56) cannot fuse its top, the last case has two views."""
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    T = 3
    ws = [stp_weights(_config(H, W, T, 1), seed=3 + v) for v in range(ncam)]
    preds = []
    for nd in (0, 1):
        hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
                  sequence_length=T + 2, n_context=2, ncam=ncam, transformation='stp')
        preds.append(HipVPredEvaluation('', hp).restore(ws if ncam > 1 else ws[0]))
    p0, p1 = preds
    assert p0.frames_only is True and p1.frames_only is False and isinstance(p0.cfg, StpConfig) and p0.cfg.ndesig == 0
    rs = np.random.RandomState(H + W + M + ncam)
    ctx0 = {'context_frames': rs.randint(0, 256, (3, ncam, H, W, 3)).astype(np.uint8),
            'context_actions': rs.normal(0, 0.05, (2, 4)), 'context_states': rs.normal(0, 0.1, (3, 5))}
    d = np.zeros((2, ncam, H, W, 1), np.float32)
    d[:, :, H // 3, W // 2, 0] = 1.
    actions = rs.normal(0, 0.1, (M, T, 4))
    want = p1(dict(ctx0, context_pixel_distributions=d), {'actions': actions})
    assert p1.device_status() == 0
    assert np.ptp(want['predicted_frames']) > 0.1 and np.isfinite(want['predicted_frames']).all()
    assert np.abs(want['predicted_frames'][0] - want['predicted_frames'][1]).max() > 0        # the actions matter
    for persistent, fuse in ((1, 1), (1, 0), (0, 1)):
        p0.set_persistent(persistent)
        p0.set_fuse_top(fuse)
        for rep in range(2):                    # the second call finds the context (and the shared units) cached
            got = p0(ctx0, {'actions': actions})
            assert p0.device_status() == 0
            assert got['predicted_pixel_distributions'] is None
            np.testing.assert_array_equal(got['predicted_frames'], want['predicted_frames'])
            np.testing.assert_array_equal(got['predicted_states'], want['predicted_states'])
        p0._ctx_key = None


# ------------------------------------------------------------------------------------------ planning
PLAN_SEED = 1      # weights seed of the planning call, chosen on the CPU from the helper alone: see the test


def plan_with(predictor_class):
    """One ``PixelCostController`` planning call (32 x 32, 40 samples, horizon 5, 2 CEM iterations) -> (result, elites, ctrl)."""
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    ag = {'adim': 4, 'sdim': 5, 'image_height': 32, 'image_width': 32}
    base = {'num_samples': 40, 'iterations': 2, 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, 32, 32, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController(dict(ag), dict(base, predictor_class=predictor_class), 0, 1)
        ctrl.reset()
        np.random.seed(0)
        ctrl.act(t=0, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[8, 24]], images=frames[:1], state=states[:1])
        out = ctrl.act(t=1, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[8, 24]], images=frames, state=states)
    return out, ctrl._best_indices.copy(), ctrl


def plan_weights(seed):
    return lambda cfg: stp_weights(cfg, seed)


def elite_gaps(result):
    """Per CEM iteration: the oracle's score gap at the elite boundary (K = 10) over the score tolerance (rtol 1e-5)."""
    out = []
    for itr in range(2):
        s = result['plan_stat']['scores_itr%d' % itr]
        out.append(np.diff(np.sort(s))[9] / (1e-5 * np.abs(s).max()))
    return out


def test_one_planning_call_selects_the_oracles_elites():
    """``PixelCostController`` driven by the HIP predictor and by the helper oracle (host cost path).  Iteration 2 samples from
    the elites of iteration 1, so equal final elites and actions mean both iterations selected identically.  ``PLAN_SEED``
    was chosen on the CPU from the oracle alone (``profiles/stp.txt`` section 1): its gap at the elite boundary (K = 10)
    exceeds four times the score tolerance (rtol 1e-5) in both iterations, so a result inside the tolerance cannot move a
    candidate across the boundary."""
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    factory = plan_weights(PLAN_SEED)

    class HipStp(HipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(HipStp, self).__init__(model_path, dict(hparams, transformation='stp'), n_gpus, first_gpu)

        def restore(self, weights=None):
            return super(HipStp, self).restore(factory(self.cfg) if weights is None else weights)

    ora, ora_idx, _ = plan_with(make_stp_predictor_class(factory))
    hip, hip_idx, ctrl = plan_with(HipStp)
    gaps = elite_gaps(ora)
    for itr in range(2):
        key = 'scores_itr%d' % itr
        s_ora, s_hip = ora['plan_stat'][key], hip['plan_stat'][key]
        print('stp planning itr %d: score rel err %.3g, oracle gap at the boundary %.1f x tolerance'
              % (itr, np.abs(s_hip / s_ora - 1).max(), gaps[itr]))
        assert gaps[itr] > 4, 'PLAN_SEED gives an ambiguous elite boundary in iteration %d' % itr
        np.testing.assert_allclose(s_hip, s_ora, rtol=1e-5)
    np.testing.assert_array_equal(hip_idx, ora_idx)
    np.testing.assert_array_equal(hip['actions'], ora['actions'])
    assert ctrl.predictor.device_status() == 0
