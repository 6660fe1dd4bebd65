"""GPU: the appearance-flow predictor (``CdnaConfig(transformation='flow')``) through the C ABI against the
helper oracle of ``tests/helpers/oracle_appflow.py``, against closed forms, and against itself over the three launch routes.

Bounds of the parity tests are those of ``test_gpu_parity.py::test_rollout_matches_oracle``: frames 1e-5, distributions 2e-5
of the plane maximum, states 1e-6, scores rtol 1e-5, planes sum to 1 within 2e-6.  Flow meets them as they are (measured:
frames <= 3.0e-6, distributions <= 4.5e-6, scores <= 1.9e-7; ``profiles/appflow.txt`` lists every case), so no bound was
derived from the float64 helper.
"""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                           # noqa: E402
from tests.helpers.oracle_appflow import OracleAppflow, make_appflow_predictor_class       # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights         # noqa: E402


def _config(H, W, T, nd, n_context=2):
    return CdnaConfig(height=H, width=W, ndesig=nd, sequence_length=T + n_context, n_context=n_context,
                      transformation='flow')


def _predictor(H, W, T, nd, bs, seed=3, n_context=2, weights=None):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + n_context, n_context=n_context, transformation='flow')
    pred = HipVPredEvaluation('', hp)
    assert pred.cfg.transformation == 'flow' and pred.cfg.layer_spec == 2
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


def _oracle(weights, ctx, actions, dtype=torch.float32):
    return OracleAppflow(weights, dtype).rollout(ctx['context_frames'], ctx['context_actions'],
                                                 ctx['context_pixel_distributions'], ctx['context_states'], actions)


def _check_parity(pred, weights, ctx, actions, goal, label):
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
    print('appflow parity %s: frames %.3g  distrib/planemax %.3g  states %.3g  scores rel %.3g  |sum - 1| %.3g'
          % (label, err_f, err_d, err_s, err_c, err_sum))
    assert err_f <= 1e-5
    assert err_d <= 2e-5
    assert err_s <= 1e-6
    np.testing.assert_allclose(scores, want, rtol=1e-5)
    np.testing.assert_allclose(per_task, want_pt, rtol=1e-5)
    own, _ = pixel_cost.eval_pixel_cost(got['predicted_pixel_distributions'], goal, 10.)
    np.testing.assert_allclose(scores, own, rtol=2e-6)
    assert err_sum <= 2e-6
    assert pred.device_status() == 0


@pytest.mark.parametrize('H,W,T,M,nd,nc', [(32, 32, 2, 5, 1, 2), (48, 64, 2, 5, 2, 2), (64, 64, 2, 3, 4, 2),
                                           (40, 56, 2, 4, 1, 2),          # a shape whose top cannot be fused: two phases
                                           (32, 32, 2, 4, 1, 1)])         # one context frame
def test_rollout_matches_oracle(H, W, T, M, nd, nc):
    pred, weights = _predictor(H, W, T, nd, bs=M, n_context=nc)
    rs = np.random.RandomState(H + W + T + M + nc)
    ctx = _context(H, W, nd, rs, hist=3 if nc == 2 else 1)
    if nc == 1:
        ctx['context_pixel_distributions'] = ctx['context_pixel_distributions'][:1]
        ctx['context_actions'] = np.zeros((0, 4))
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(-2, max(H, W) + 2, (1, nd, 2))          # goals may lie off-image
    _check_parity(pred, weights, ctx, actions, goal, '%dx%d nd %d nc %d' % (H, W, nd, nc))


def test_large_flows_clamp_at_every_border():
    """``flow/b`` drawn from +-0.75 min(H, W): most warps leave the image on some side, so the clamps of both coordinates at
    both ends are on the path of every pixel row and column."""
    H = W = 32
    T, M, nd = 2, 5, 2
    cfg = _config(H, W, T, nd)
    weights = CdnaWeights.random(cfg, seed=11, bias_scale=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(12)
    weights.tensors['flow/b'][:] = rs.uniform(-0.75 * min(H, W), 0.75 * min(H, W), 18).astype(np.float32)
    fb = weights.tensors['flow/b']
    assert fb[0::2].min() < -8 and fb[0::2].max() > 8 and fb[1::2].min() < -8 and fb[1::2].max() > 8
    pred, _ = _predictor(H, W, T, nd, bs=M, weights=weights)
    ctx = _context(H, W, nd, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, H, (1, nd, 2))
    _check_parity(pred, weights, ctx, actions, goal, 'large flows 32x32 nd 2')


def _translate(img, dx, dy):
    """Clamped bilinear translate of ``img [H, W, C]`` by one shift, NumPy float64: out[y, x] = img(x + dx, y + dy)."""
    H, W = img.shape[:2]
    x = np.clip(np.arange(W) + dx, 0, W - 1)
    y = np.clip(np.arange(H) + dy, 0, H - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (x - x0)[None, :, None], (y - y0)[:, None, None]
    img = img.astype(np.float64)
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


@pytest.mark.parametrize('shift,desig', [((1.5, -0.25), (10, 12)), ((40., -40.), (0, 31))])
def test_closed_form_translation(shift, desig):
    """No oracle: zero ``flow/w`` and ``masks/w``, ``masks/b`` = +40 on channel 2 (the mask of warp 0 is 1.0 in fp32, the
    others 4e-18), ``flow/b`` gives warp 0 one shift for every pixel.  The first predicted frame is then the bilinear
    translate of the last context frame and the one-hot distribution splits into the four tap weights; with the shift
    (40, -40) every pixel takes the value of the corner (row 0, column W - 1) it clamps to."""
    H = W = 32
    T, M = 2, 3
    cfg = _config(H, W, T, 1)
    weights = CdnaWeights.random(cfg, seed=7, bias_scale=0.05, ln_jitter=0.1)
    t = weights.tensors
    t['flow/w'][:] = 0
    t['masks/w'][:] = 0
    t['masks/b'][:] = 0
    t['masks/b'][2] = 40.
    t['flow/b'][:] = np.random.RandomState(1).uniform(-5, 5, 18)        # warps 1..8: any flow, their masks are 4e-18
    t['flow/b'][0], t['flow/b'][1] = shift
    pred, _ = _predictor(H, W, T, 1, bs=M, weights=weights)
    rs = np.random.RandomState(21)
    ctx = _context(H, W, 1, rs, desig=np.array([[desig]]))
    actions = rs.normal(0, 0.1, (M, T, 4))
    got = pred(ctx, {'actions': actions})
    last = ctx['context_frames'][-1, 0].astype(np.float32) / np.float32(255.)
    want_f = _translate(last, *shift)
    err = np.abs(got['predicted_frames'][:, 0, 0] - want_f[None]).max()
    print('appflow closed form shift %s: first frame err %.3g' % (shift, err))
    assert err <= 1e-6
    onehot = np.zeros((H, W, 1))
    onehot[desig] = 1.
    want_d = _translate(onehot, *shift)
    d0 = got['predicted_pixel_distributions'][:, 0, 0]
    if shift == (1.5, -0.25):
        r, c = desig        # pixel (y, x) samples (x + 1.5, y - 0.25): taps (y - 1 | y, x + 1 | x + 2), fx 0.5, fy 0.75
        expect = {(r + 1, c - 1): 0.125, (r + 1, c - 2): 0.125, (r, c - 1): 0.375, (r, c - 2): 0.375}
        assert {k: v for k, v in np.ndenumerate(want_d[..., 0]) if v} == expect
        assert all(np.abs(d0[:, y, x, 0] - v).max() <= 1e-6 for (y, x), v in expect.items())
        assert (d0 > 1e-9).sum() == 4 * M
    else:
        assert np.all(want_f == last[0, W - 1]) and np.all(want_d == 1.)
        want_d = want_d / want_d.sum()      # every pixel samples the designated corner: a uniform plane
    assert np.abs(d0 - want_d[None]).max() <= 1e-6
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
        got = pred(ctx, {'actions': actions})
        sp, _ = pred.score(ctx, {'actions': actions[perm]}, goal)
        gp = pred(ctx, {'actions': actions[perm]})
        np.testing.assert_array_equal(sp, s[perm])
        np.testing.assert_array_equal(gp['predicted_frames'], got['predicted_frames'][perm])
        np.testing.assert_array_equal(gp['predicted_pixel_distributions'], got['predicted_pixel_distributions'][perm])
        outs.append((s, pt, got['predicted_frames'], got['predicted_pixel_distributions'], got['predicted_states']))
        pred._ctx_key = None                    # upload the context again: the next route computes the shared units itself
    assert np.isfinite(outs[0][0]).all() and np.ptp(outs[0][0]) > 0
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)
    assert pred.device_status() == 0


PLAN_SEED = 8      # weights seed of the planning call, chosen on the CPU: see the test


def test_one_planning_call_selects_the_oracles_elites():
    """``PixelCostController`` at 32 x 32, 40 samples, horizon 5, 2 CEM iterations, driven by the HIP predictor and by the
    helper oracle (host cost path).  Iteration 2 samples from the elites of iteration 1, so equal final elites and actions
    mean both iterations selected identically.  ``PLAN_SEED`` was chosen on the CPU from the oracle alone: its gap at the
    elite boundary (K = 10) exceeds four times the score tolerance (rtol 1e-5) in both iterations, so a result inside the
    tolerance cannot move a candidate across the boundary."""
    from visual_foresight_amd.policy.cem_controllers import PixelCostController
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    ag = {'adim': 4, 'sdim': 5, 'image_height': 32, 'image_width': 32}
    base = {'num_samples': 40, 'iterations': 2, 'repeat': 1, 'rejection_sampling': False, 'verbose': False}
    factory = lambda cfg: CdnaWeights.random(cfg, seed=PLAN_SEED, bias_scale=0.05, ln_jitter=0.1)
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, 32, 32, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))

    class HipFlow(HipVPredEvaluation):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(HipFlow, self).__init__(model_path, dict(hparams, transformation='flow'), n_gpus, first_gpu)

        def restore(self, weights=None):
            return super(HipFlow, self).restore(factory(self.cfg) if weights is None else weights)

    def run(predictor_class):
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = PixelCostController(dict(ag), dict(base, predictor_class=predictor_class), 0, 1)
            ctrl.reset()
            np.random.seed(0)
            ctrl.act(t=0, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[8, 24]], images=frames[:1], state=states[:1])
            out = ctrl.act(t=1, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[8, 24]], images=frames, state=states)
        return out, ctrl._best_indices.copy(), ctrl

    ora, ora_idx, _ = run(make_appflow_predictor_class(factory))
    hip, hip_idx, ctrl = run(HipFlow)
    for itr in range(2):
        key = 'scores_itr%d' % itr
        s_ora, s_hip = ora['plan_stat'][key], hip['plan_stat'][key]
        gap = np.diff(np.sort(s_ora))[9]
        print('appflow planning itr %d: score rel err %.3g, oracle gap at the boundary %.3g (x tolerance: %.1f)'
              % (itr, np.abs(s_hip / s_ora - 1).max(), gap, gap / (1e-5 * np.abs(s_ora).max())))
        assert gap > 4 * 1e-5 * np.abs(s_ora).max(), 'PLAN_SEED gives an ambiguous elite boundary in iteration %d' % itr
        np.testing.assert_allclose(s_hip, s_ora, rtol=1e-5)
    np.testing.assert_array_equal(hip_idx, ora_idx)
    np.testing.assert_array_equal(hip['actions'], ora['actions'])
    assert ctrl.predictor.device_status() == 0
