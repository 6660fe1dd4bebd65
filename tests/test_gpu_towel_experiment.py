"""GPU: the reference's towel-folding experiment (``experiments/sawyer/towel_classifier``) end to end on the engine, at its
own size: 48 x 64 images, one view, ``adim`` 4, the agent's five state dimensions plus the three ``state_append`` constants,
18 samples, 5 action steps held 3 times, two context frames, appearance-flow compositing (``'model': 'appflow'``), no
designated pixel (``FramesOnlyHipVPredEvaluation``), ``ClassifierController`` with ``FoldingCEMSampler``.

The folding sampler rolls action magnitudes no other GPU test does: lifts of exactly +-1/3 in every scripted step and xy
shifts up to 1/5 (the Gaussian sampler's standard deviation is 0.05).

1. The frames of the 18 first-iteration candidates against the appearance-flow oracle.
2. One literal planning call against the same controller on the CPU oracle predictor and the float64 oracle scorer.
3. The same planning call with ``HipVPredEvaluation`` (one dummy distribution) and with the frames-only class: the same bits.

Measured figures: ``profiles/towel_experiment.txt``.
"""
import contextlib
import io
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.helpers import folding_fixtures as fx                                            # noqa: E402
from tests.helpers import oracle_frame_scorer as ora                                        # noqa: E402
from tests.helpers.oracle_appflow import OracleAppflow, make_appflow_predictor_class        # noqa: E402
from visual_foresight_amd.hparams import HParams                                            # noqa: E402
from visual_foresight_amd.policy.cem_controllers.samplers.folding_sampler import FoldingCEMSampler      # noqa: E402
from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController      # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights         # noqa: E402

H, W, M, T, K = 48, 64, 18, 15, 10
APPENDED = [0.41, 0.25, 0.166]
AG = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
# frames, absolute: the bound ``tests/test_gpu_appflow.py`` (``_check_parity``: ``err_f <= 1e-5``) applies to its 48 x 64
# case, which is also that of ``test_gpu_frames_only.py::test_frames_match_the_oracle_run_with_a_dummy_distribution``
FRAME_TOL = 1e-5
# the two constants of ``tests/test_gpu_learned_cost.py::test_planning_elites_match_oracle_predictor_and_scorer``
HEAD_FACTOR = 8.0
FRAME_PARITY = 5e-7
# scorer weights of the planning call: chosen on the CPU oracle alone (see test 2)
SCORER_SEED, SCORER_BIAS = 12, 0.2


def weights_factory(cfg):
    return CdnaWeights.random(cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)


def observations():
    """Two uint8 frames and the agent's states; xy of the last state is a corner of the unit square, so that carries to
    places more than 0.6 away - most of the square - have means beyond the 0.2 clip."""
    rs = np.random.RandomState(6)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    states[-1, :2] = [1.0, 0.0]
    return frames, states


def towel_policy(golden_dir, conf_path):
    """The sawyer towel ``policy`` dict of the fixture with the two home-directory paths replaced (the caller sets
    ``predictor_class``, the third and last key a test may set)."""
    with open(os.path.join(golden_dir, 'folding_sampler.json')) as f:
        case = json.load(f)['towel']['sawyer']
    assert case['agent'] == {'T': 15, 'image_height': H, 'image_width': W} and case['conf']['sdim'] == 5 + len(APPENDED)
    pol = {k: FoldingCEMSampler if v == 'class:FoldingCEMSampler' else v for k, v in case['policy'].items()}
    assert pol['sampler'] is FoldingCEMSampler and pol['state_append'] == APPENDED and pol['num_samples'] == M
    with open(conf_path, 'w') as f:
        json.dump({'seed': SCORER_SEED, 'bias_scale': SCORER_BIAS}, f)
    pol['classifier_conf_path'] = conf_path
    del pol['classifier_restore_path']
    return pol


def _flow(base):
    """``base`` with ``transformation='flow'`` and the weights of ``weights_factory`` (the subclassing of
    ``tests/test_gpu_frames_only.py::_with_transformation``)."""
    class Selected(base):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(Selected, self).__init__(model_path, dict(hparams, transformation='flow'), n_gpus, first_gpu)

        def restore(self, weights=None):
            return super(Selected, self).restore(weights_factory(self.cfg) if weights is None else weights)
    return Selected


def first_iteration_candidates(states):
    hp = fx.hp_for(HParams, FoldingCEMSampler, **fx.TOWEL_STD)
    np.random.seed(7)
    actions = FoldingCEMSampler(hp, 4, 5).sample_initial_actions(1, M, states[-1])
    assert actions.shape == (M, T, 4)
    assert np.abs(actions[:, :, :2]).max() == 0.2 and np.abs(actions[:, :, 2]).max() == 1. / 3      # both clips are reached
    return actions


def oracle_frames(actions, frames, states8, dtype):
    cfg = CdnaConfig(height=H, width=W, adim=4, sdim=8, ndesig=1, sequence_length=T + 2, transformation='flow')
    dummy = np.zeros((2, 1, H, W, 1), np.float32)
    dummy[:, :, H // 2, W // 2, :] = 1.
    f, _, s = OracleAppflow(weights_factory(cfg), dtype).rollout(frames, np.zeros((1, 4)), dummy, states8, actions)
    return f, s


# ---------------------------------------------------------------------------------------- 1. frames
def test_frames_at_the_folding_samplers_magnitudes_match_the_oracle():
    """Float32 oracle against float64 oracle on these inputs, measured on the CPU before any device run: frames 1.68e-6,
    states 2.63e-7 (largest |state| 2.05) - inside the tolerance, so the float32 oracle is a fit reference at these
    magnitudes.  The float64 run takes twice as long as the float32 one and is not repeated here.
    One MI355X (profiles/towel_experiment.txt): max |device - float32 oracle| frames 3.29e-6, states 4.77e-7."""
    from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation
    torch.set_num_threads(min(16, torch.get_num_threads()))
    frames, states = observations()
    states8 = np.concatenate((states, np.tile(APPENDED, (2, 1))), axis=1)
    actions = first_iteration_candidates(states)
    hp = dict(designated_pixel_count=1, run_batch_size=M, adim=4, sdim=8, image_height=H, image_width=W,
              sequence_length=T + 2)
    pred = _flow(FramesOnlyHipVPredEvaluation)('', hp).restore()
    assert pred.frames_only and pred.cfg.transformation == 'flow' and pred.cfg.sdim == 8
    ctx = {'context_frames': frames, 'context_actions': np.zeros((1, 4)), 'context_states': states8}
    got = pred(ctx, {'actions': actions})
    assert pred.device_status() == 0
    want_f, want_s = oracle_frames(actions, frames, states8, torch.float32)
    err_f = np.abs(got['predicted_frames'] - want_f).max()
    err_s = np.abs(got['predicted_states'] - want_s).max()
    print('towel frames 48x64, 18 folding candidates x T15: max |device - float32 oracle| frames %.3g (tolerance %g), states '
          '%.3g (largest |state| %.3g)' % (err_f, FRAME_TOL, err_s, np.abs(want_s).max()))
    assert np.isfinite(got['predicted_frames']).all() and np.ptp(want_f) > 0.1
    assert np.abs(want_f[0] - want_f[M - 1]).max() > 1e-3                       # the actions matter
    assert err_f <= FRAME_TOL


# ---------------------------------------------------------------------------------------- 2. one planning call
def plan(cls, predictor_class, pol):
    frames, states = observations()
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = cls(dict(AG), dict(pol, predictor_class=predictor_class), 0, 1)
        ctrl.reset()
        np.random.seed(0)
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1])
        t0 = time.perf_counter()
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states)
        ctrl.plan_seconds = time.perf_counter() - t0
    return ctrl, out


class OnOracle(ClassifierController):
    """The controller with the float64 oracle scorer; remembers the oracle predictor's frames of iteration 0."""
    seen = None

    def _build_scorer(self):
        host = super(OnOracle, self)._build_scorer()
        return ora.OracleFrameScorer(host.weights, host.cfg, self._n_cam)

    def _host_scores(self, gen_images, goal_enc):
        if self.seen is None:
            self.seen = np.asarray(gen_images)
        return super(OnOracle, self)._host_scores(gen_images, goal_enc)


def oracle_plan(pol):
    return plan(OnOracle, make_appflow_predictor_class(weights_factory), pol)


def score_cap(oc, ora_out):
    """The cap on ``max |device - oracle|`` of a score, from the CPU alone, exactly as
    ``test_planning_elites_match_oracle_predictor_and_scorer`` computes it."""
    gen = oc.seen
    n, t = gen.shape[:2]

    def oracle_scores(frames32, dtype=torch.float64):
        enc = ora.forward_views(oc.scorer.weights['frames'], frames32.reshape((n * t,) + frames32.shape[2:]),
                                oc.scorer.cfg.input_scale, dtype).reshape(n, t, 1, -1)
        raw = ora.classifier_raw(enc)
        return ora.weight_scores(raw, oc._hp.finalweight), raw, enc

    s0, raw0, enc64 = oracle_scores(gen)
    np.testing.assert_allclose(s0, ora_out['plan_stat']['scores_itr0'], rtol=1e-12)
    prs = np.random.RandomState(7)

    def shifts():
        yield np.float32(FRAME_PARITY)
        yield np.float32(-FRAME_PARITY)
        for _ in range(8):
            yield np.where(prs.randint(0, 2, gen.shape) > 0, np.float32(FRAME_PARITY), np.float32(-FRAME_PARITY))

    perturbed = max(np.abs(oracle_scores(gen + d)[0] - s0).max() for d in shifts())
    enc32 = oracle_scores(gen, torch.float32)[2]
    head_bound = HEAD_FACTOR * np.abs(enc32 - enc64).max() / np.abs(enc64).max()
    cap = 10 * (perturbed + head_bound * np.abs(raw0).max())
    print('towel: frame-parity perturbation moves the oracle score by at most %.3g; item-6 bound %.3g x largest |raw| %.3g; '
          'cap %.3g' % (perturbed, head_bound, np.abs(raw0).max(), cap))
    return cap


def boundary(s_ora):
    srt = np.sort(s_ora)
    return srt[K] - srt[K - 1], srt[-1] - srt[0]


def test_one_literal_planning_call_selects_the_oracles_elites(golden_dir, tmp_path):
    """The towel ``policy`` dict on the engine (``FramesOnlyHipVPredEvaluation`` with flow compositing + ``HipFrameScorer``)
    against the same dict on ``make_appflow_predictor_class`` + ``OracleFrameScorer``, both under ``np.random.seed(0)``: per
    iteration the same 10 elites of 18 (``selection_frac`` 0.05 -> ``minimum_selection``), ``diff <= cap`` and
    ``gap > 4 * diff`` (diff: max |device - oracle| of a score; gap: the oracle's score difference at the K / K+1 boundary);
    at the end the same ``_best_indices`` and the same action.  The method, the cap included, is that of
    ``tests/test_gpu_learned_cost.py::test_planning_elites_match_oracle_predictor_and_scorer``.

    The scorer's seed and ``bias_scale`` were chosen on the CPU oracle alone, before any device run, so that the gap is at
    least 1e-2 of the score range in all three iterations: of the seeds 1 .. 13 at ``bias_scale`` 0.2, five meet that
    (3, 4, 6, 11, 12); 12 has the widest smallest gap.

    Figures, CPU oracle (scorer seed 12, bias_scale 0.2): gap / score range 3.95e-2, 6.93e-2, 1.54e-1 in iterations 0, 1, 2
    (gaps 2.16e-4, 1.90e-4, 2.25e-4; ranges 5.47e-3, 2.74e-3, 1.46e-3); frame-parity perturbation moves the oracle score by
    at most 3.41e-7, item-6 bound 3.75e-6 x largest |raw| 0.716 -> cap 3.03e-5.  One oracle planning call: 11 s on 16 threads.
    One MI355X (profiles/towel_experiment.txt): max |device - oracle| 2.41e-7, 1.79e-7, 1.86e-7 in iterations 0, 1, 2; the
    cap came to 3.57e-5 there (its item-6 term is the float32 error of PyTorch's CPU convolutions, which depends on the
    host: 4.52e-6 against 3.75e-6); the same elites, ``_best_indices`` and action; one planning call 0.08 s on the engine."""
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation
    torch.set_num_threads(min(16, torch.get_num_threads()))
    pol = towel_policy(golden_dir, str(tmp_path / 'scorer_conf.json'))
    oc, ora_out = oracle_plan(pol)
    assert oc.predictor.cfg.sdim == 8 and oc._elite_count() == K
    cap = score_cap(oc, ora_out)

    hc, hip_out = plan(ClassifierController, _flow(FramesOnlyHipVPredEvaluation), pol)
    assert hasattr(hc.predictor, 'score_frames') and isinstance(hc.scorer, HipFrameScorer)
    assert hc.predictor.frames_only and hc.predictor.cfg.sdim == 8 and hc.predictor.cfg.transformation == 'flow'
    assert hc.predictor.device_status() == 0
    print('towel: one planning call on the engine (18 x T15, 3 iterations) took %.3g s, on the CPU oracle %.3g s'
          % (hc.plan_seconds, oc.plan_seconds))
    for itr in range(3):
        key = 'scores_itr%d' % itr
        s_hip, s_ora = hip_out['plan_stat'][key], ora_out['plan_stat'][key]
        assert s_hip.shape == s_ora.shape == (M,)
        gap, span = boundary(s_ora)
        diff = np.abs(s_hip - s_ora).max()
        print('towel itr %d: max |device - oracle| %.3g (cap %.3g), oracle gap %.3g = %.3g of the score range %.3g'
              % (itr, diff, cap, gap, gap / span, span))
        assert gap >= 1e-2 * span, 'fixture seeds give a narrow elite boundary'
        assert gap > 4 * diff, 'fixture seeds give an ambiguous elite boundary'
        assert diff <= cap
        np.testing.assert_array_equal(np.sort(np.argsort(s_hip)[:K]), np.sort(np.argsort(s_ora)[:K]))
    np.testing.assert_array_equal(hc._best_indices, oc._best_indices)
    np.testing.assert_array_equal(hip_out['actions'], ora_out['actions'])


# ---------------------------------------------------------------------------------------- 3. either predictor class
def test_the_planning_call_is_the_same_with_either_predictor_class(golden_dir, tmp_path):
    """``test_gpu_frames_only.py::test_a_planning_call_is_the_same_with_either_predictor_class`` with the towel dict: the
    folding sampler and ``state_append``."""
    from visual_foresight_amd.video_prediction.hip_predictor import FramesOnlyHipVPredEvaluation, HipVPredEvaluation
    pol = towel_policy(golden_dir, str(tmp_path / 'scorer_conf.json'))
    (c0, o0), (c1, o1) = (plan(ClassifierController, _flow(base), pol) for base in (FramesOnlyHipVPredEvaluation,
                                                                                    HipVPredEvaluation))
    assert c0.predictor.frames_only and c0.predictor.cfg.ndesig == 0 and not c1.predictor.frames_only
    for c in (c0, c1):
        assert c.predictor.device_status() == 0 and c.predictor.cfg.sdim == 8 and c.predictor.cfg.transformation == 'flow'
    for itr in range(3):
        s0, s1 = o0['plan_stat']['scores_itr%d' % itr], o1['plan_stat']['scores_itr%d' % itr]
        assert s0.shape == (M,) and len(np.unique(s0)) == M
        np.testing.assert_array_equal(s0, s1)
    np.testing.assert_array_equal(c0._best_indices, c1._best_indices)
    np.testing.assert_array_equal(o0['actions'], o1['actions'])
    np.testing.assert_array_equal(c0.cost_perstep, c1.cost_perstep)
