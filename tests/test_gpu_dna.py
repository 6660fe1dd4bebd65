"""GPU: the DNA predictor (``DnaConfig``) through the C ABI against the helper oracle of
``tests/helpers/oracle_dna.py``, against closed forms, and against itself over the three launch routes.

Bounds of the parity tests are those of ``test_gpu_parity.py::test_rollout_matches_oracle``: frames 1e-5, distributions 2e-5
of the plane maximum, states 1e-6, scores rtol 1e-5, device scores against the host cost of the device's distributions 2e-6,
planes sum to 1 within 2e-6.  The float32 helper's own distance to its float64 mode at these shapes (measured on the CPU,
``profiles/dna.txt`` section 1) is at most 1.1e-6 for frames, 1.9e-6 of the plane maximum for distributions, 3.6e-8 for
states and 1.3e-7 for scores: below a quarter of each bound.
"""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                           # noqa: E402
from tests.helpers.oracle_dna import OracleDna, make_dna_predictor_class                   # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaWeights                    # noqa: E402
from visual_foresight_amd.video_prediction.dna_arch import DnaConfig                       # noqa: E402


def _config(H, W, T, nd, n_context=2):
    return DnaConfig(height=H, width=W, ndesig=nd, sequence_length=T + n_context, n_context=n_context)


def _predictor(H, W, T, nd, bs, seed=3, n_context=2, weights=None):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + n_context, n_context=n_context, transformation='dna')
    pred = HipVPredEvaluation('', hp)
    assert isinstance(pred.cfg, DnaConfig) and pred.cfg.layer_spec == 3 and pred.cfg.num_masks == 1
    if weights is None:
        weights = CdnaWeights.random(_config(H, W, T, nd, n_context), seed=seed, bias_scale=0.05, ln_jitter=0.1)
    pred.restore(weights)
    return pred, weights


def _context(H, W, nd, rs, hist=3, desig=None):
    if desig is None:
        desig = np.stack([rs.randint(0, H, (1, nd)), rs.randint(0, W, (1, nd))], axis=-1)
    return {'context_frames': rs.randint(0, 256, (hist, 1, H, W, 3)).astype(np.uint8),
            'context_actions': rs.normal(0, 0.05, (hist - 1, 4)),
            'context_states': rs.normal(0, 0.1, (hist, 5)),
            'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, 2, 1, H, W, nd)}


PARITY_CASES = [(32, 32, 2, 5, 1, 2), (48, 64, 2, 5, 2, 2), (64, 64, 2, 3, 4, 2),
                (40, 56, 2, 4, 1, 2),          # a shape whose top cannot be fused: two phases
                (32, 32, 2, 4, 1, 1)]          # one context frame


def parity_inputs(H, W, T, M, nd, nc):
    """Weights and inputs of one parity case (also used on the CPU to measure the helper against its float64 mode)."""
    weights = CdnaWeights.random(_config(H, W, T, nd, nc), seed=3, bias_scale=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(H + W + T + M + nc)
    ctx = _context(H, W, nd, rs, hist=3 if nc == 2 else 1)
    if nc == 1:
        ctx['context_pixel_distributions'] = ctx['context_pixel_distributions'][:1]
        ctx['context_actions'] = np.zeros((0, 4))
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(-2, max(H, W) + 2, (1, nd, 2))          # goals may lie off-image
    return weights, ctx, actions, goal


def _oracle(weights, ctx, actions, dtype=torch.float32):
    return OracleDna(weights, dtype).rollout(ctx['context_frames'], ctx['context_actions'],
                                             ctx['context_pixel_distributions'], ctx['context_states'], actions)


@pytest.mark.parametrize('H,W,T,M,nd,nc', PARITY_CASES)
def test_rollout_matches_oracle(H, W, T, M, nd, nc):
    weights, ctx, actions, goal = parity_inputs(H, W, T, M, nd, nc)
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
    print('dna parity %dx%d nd %d nc %d: frames %.3g  distrib/planemax %.3g  states %.3g  scores rel %.3g  own cost rel %.3g  '
          '|sum - 1| %.3g' % (H, W, nd, nc, err_f, err_d, err_s, err_c, np.abs(scores / own - 1).max(), err_sum))
    assert err_f <= 1e-5
    assert err_d <= 2e-5
    assert err_s <= 1e-6
    np.testing.assert_allclose(scores, want, rtol=1e-5)
    np.testing.assert_allclose(per_task, want_pt, rtol=1e-5)
    np.testing.assert_allclose(scores, own, rtol=2e-6)
    assert err_sum <= 2e-6
    assert pred.device_status() == 0


def _shift(img, dy, dx):
    """out[y, x] = img[y + dy, x + dx], zero outside the image (``img [H, W, C]``, float64)."""
    H, W = img.shape[:2]
    out = np.zeros(img.shape, np.float64)
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    out[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    return out


def _closed_form_run(dna_b, desig):
    """32 x 32, one designated pixel, zero ``dna/w`` and ``masks/w``, ``masks/b = [0, 40]`` (mask 1 is 1.0 in fp32, mask 0
    4e-18): every pixel has the same kernel, the one ``dna/b`` spells.  -> (last context frame, one-hot plane, first predicted
    frames [M, H, W, 3], first predicted distributions [M, H, W], predictor)."""
    H = W = 32
    T, M = 2, 3
    weights = CdnaWeights.random(_config(H, W, T, 1), seed=7, bias_scale=0.05, ln_jitter=0.1)
    t = weights.tensors
    t['dna/w'][:] = 0
    t['masks/w'][:] = 0
    t['masks/b'][:] = [0., 40.]
    t['dna/b'][:] = np.asarray(dna_b, np.float32)
    pred, _ = _predictor(H, W, T, 1, bs=M, weights=weights)
    rs = np.random.RandomState(21)
    ctx = _context(H, W, 1, rs, desig=np.array([[desig]]))
    got = pred(ctx, {'actions': rs.normal(0, 0.1, (M, T, 4))})
    last = ctx['context_frames'][-1, 0].astype(np.float32) / np.float32(255.)
    onehot = np.zeros((H, W, 1))
    onehot[desig] = 1.
    return last.astype(np.float64), onehot, got['predicted_frames'][:, 0, 0], got['predicted_pixel_distributions'][:, 0, 0, :, :, 0], pred


@pytest.mark.parametrize('tap,desig', [((0, 4), (15, 17)), ((4, 0), (16, 14))])
def test_closed_form_one_hot_tap_shifts_the_frame(tap, desig):
    """(a) ``dna/b`` = -1 except +1 at one tap: the kernel is that tap (the dead taps weigh 1e-12), so the first predicted
    frame is the last context frame shifted by ``(dy - 2, dx - 2)`` with zero rows and columns entering, and the one-hot
    distribution moves by the opposite shift.  Taps (0, 4) and (4, 0) shift by two pixels towards opposite corners: across
    the edges of the 16-pixel tiles, with zeros entering at two image borders each; the designated pixels sit beside a tile
    corner and cross it."""
    dy, dx = tap
    b = -np.ones(25)
    b[5 * dy + dx] = 1.
    last, onehot, f0, d0, pred = _closed_form_run(b, desig)
    want_f = _shift(last, dy - 2, dx - 2)
    assert (want_f[:2] == 0).all() or (want_f[-2:] == 0).all()
    assert (want_f[:, :2] == 0).all() or (want_f[:, -2:] == 0).all()
    err = np.abs(f0 - want_f[None]).max()
    want_d = _shift(onehot, dy - 2, dx - 2)[..., 0]
    r, c = desig[0] - (dy - 2), desig[1] - (dx - 2)
    assert want_d[r, c] == 1. and want_d.sum() == 1. and (r // 16, c // 16) != (desig[0] // 16, desig[1] // 16)
    err_d = np.abs(d0 - want_d[None]).max()
    print('dna closed form tap %s: first frame err %.3g, distribution err %.3g' % (tap, err, err_d))
    assert err <= 1e-6
    assert err_d <= 1e-6
    assert pred.device_status() == 0


def test_closed_form_two_taps_split_the_one_hot():
    """(b) ``dna/b`` = 3 and 1 at two taps, -1 elsewhere: the kernel is 0.75 / 0.25 on those taps."""
    b = -np.ones(25)
    (dy0, dx0), (dy1, dx1) = (1, 3), (4, 2)
    b[5 * dy0 + dx0], b[5 * dy1 + dx1] = 3., 1.
    desig = (15, 16)
    last, onehot, f0, d0, pred = _closed_form_run(b, desig)
    want_f = 0.75 * _shift(last, dy0 - 2, dx0 - 2) + 0.25 * _shift(last, dy1 - 2, dx1 - 2)
    want_d = (0.75 * _shift(onehot, dy0 - 2, dx0 - 2) + 0.25 * _shift(onehot, dy1 - 2, dx1 - 2))[..., 0]
    assert want_d[desig[0] - (dy0 - 2), desig[1] - (dx0 - 2)] == 0.75 and want_d[desig[0] - (dy1 - 2), desig[1] - (dx1 - 2)] == 0.25
    err, err_d = np.abs(f0 - want_f[None]).max(), np.abs(d0 - want_d[None]).max()
    print('dna closed form two taps: first frame err %.3g, distribution err %.3g' % (err, err_d))
    assert err <= 1e-6
    assert err_d <= 1e-6
    assert (d0 > 1e-9).sum() == 2 * d0.shape[0]
    assert pred.device_status() == 0


def test_closed_form_all_taps_at_the_relu_shift_is_the_box_filter():
    """(c) ``dna/b`` = -5 everywhere: every ``v_t`` is the relu shift, so the kernel is the uniform 1/25 box filter with zero
    padding - compared with a NumPy float64 box filter."""
    desig = (1, 30)                 # two border bands clip the designated pixel's box
    last, onehot, f0, d0, pred = _closed_form_run(-5. * np.ones(25), desig)
    box = lambda img: sum(_shift(img, dy - 2, dx - 2) for dy in range(5) for dx in range(5)) / 25.
    want_f, want_d = box(last), box(onehot)[..., 0]
    want_d = want_d / want_d.sum()
    err, err_d = np.abs(f0 - want_f[None]).max(), np.abs(d0 - want_d[None]).max()
    print('dna closed form box filter: first frame err %.3g, distribution err %.3g' % (err, err_d))
    assert err <= 1e-6
    assert err_d <= 1e-6
    assert pred.device_status() == 0


@pytest.mark.parametrize('H,W,nd,M,T', [pytest.param(32, 32, 2, 9, 3, id='32-32-2-9'), pytest.param(64, 64, 4, 6, 3, id='64-64-4-6'),
                                        pytest.param(32, 32, 1, 3, 2, id='32-32-1-3-T2'), pytest.param(32, 32, 3, 3, 2, id='32-32-3-3-T2')])
def test_launch_routes_are_invisible_in_the_results(H, W, nd, M, T):
    """Fused top, two-phase persistent schedule and per-layer launches run the same per-pixel code on the same floats: the
    same bits for scores, frames, distributions and states - in a second call (cached context) and with every sequence
    moved to another slot of the batch.  The four cases are the four designated-pixel counts the kernels are instantiated for."""
    pred, _ = _predictor(H, W, T, nd, bs=M, seed=5)
    rs = np.random.RandomState(H + M)
    ctx = _context(H, W, nd, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, min(H, W), (1, nd, 2))
    perm = np.roll(np.arange(M), 1)
    outs = []
    for persistent, fuse in ((1, 1), (1, 0), (0, 1)):
        pred.set_persistent(persistent)
        pred.set_fuse_top(fuse)
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
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)
    assert pred.device_status() == 0


PLAN_SEED = 7      # weights seed of the planning call, chosen on the CPU from the helper alone: see the test


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
    return lambda cfg: CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)


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
    was chosen on the CPU from the oracle alone: its gap at the elite boundary (K = 10) exceeds four times the score
    tolerance (rtol 1e-5) in both iterations, so a result inside the tolerance cannot move a candidate across the boundary."""
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    factory = plan_weights(PLAN_SEED)

    class HipDna(HipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(HipDna, self).__init__(model_path, dict(hparams, transformation='dna'), n_gpus, first_gpu)

        def restore(self, weights=None):
            return super(HipDna, self).restore(factory(self.cfg) if weights is None else weights)

    ora, ora_idx, _ = plan_with(make_dna_predictor_class(factory))
    hip, hip_idx, ctrl = plan_with(HipDna)
    gaps = elite_gaps(ora)
    for itr in range(2):
        key = 'scores_itr%d' % itr
        s_ora, s_hip = ora['plan_stat'][key], hip['plan_stat'][key]
        print('dna planning itr %d: score rel err %.3g, oracle gap at the boundary %.1f x tolerance'
              % (itr, np.abs(s_hip / s_ora - 1).max(), gaps[itr]))
        assert gaps[itr] > 4, 'PLAN_SEED gives an ambiguous elite boundary in iteration %d' % itr
        np.testing.assert_allclose(s_hip, s_ora, rtol=1e-5)
    np.testing.assert_array_equal(hip_idx, ora_idx)
    np.testing.assert_array_equal(hip['actions'], ora['actions'])
    assert ctrl.predictor.device_status() == 0
