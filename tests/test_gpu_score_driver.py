"""The sharded scoring driver (``hip_predictor.score_rows``) under every cost it serves: the pixel cost, the goal-image cost
and the learned frame cost share ONE lane loop, one chunked roll-and-reduce and one scoring-call hook for the latent draws.

* a lane whose share of a call is empty, in every cost (only ``__call__`` had such a test);
* ragged chunks inside ragged lane shares;
* the latent draws of ``StochasticHipPredictor`` advance once per scoring call, refused calls included, and the ensemble
  advances its member 0 alone.

Everything is compared bit for bit with one unchunked engine: moving float64 rows is copying, not arithmetic.  Shapes are
the smallest the engine rolls (32x32, T = 2, one view, one designated pixel).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                                                   # noqa: E402
from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor      # noqa: E402
from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer                  # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation             # noqa: E402
from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor  # noqa: E402

H = W = 32
T, M = 2, 6
GOAL_PIX = np.array([[[9, 21]]])
FINALWEIGHT = 4.


def _hp(**extra):
    return dict(dict(designated_pixel_count=1, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
                     sequence_length=T + 2), **extra)


def _inputs():
    """Context (with a one-hot distribution for the pixel cost), M candidate actions and a goal image."""
    rs = np.random.RandomState(5)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib([[[14, 17]]], 2, 1, H, W, 1)}
    return ctx, rs.normal(0, 0.1, (M, T, 4)), rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32)


def _scorer(device, rolled=M):
    """The classifier-head frame scorer of ``learned_cost_rank_worker.build``, at this file's shapes."""
    return HipFrameScorer('', dict(image_height=H, image_width=W, ncam=1, max_frames=rolled * T, bias_scale=0.2,
                                   head='classifier', seed=5), device).restore()


def _pixel_cost(pred, ctx, actions, goal_image, scorer):
    s, pt = pred.score(ctx, {'actions': actions}, GOAL_PIX, finalweight=FINALWEIGHT)
    return {'score': s, 'score per task': pt}


def _goal_cost(pred, ctx, actions, goal_image, scorer):
    s, pv = pred.score_goal_image(ctx, {'actions': actions}, goal_image, steps='weighted', finalweight=FINALWEIGHT)
    return {'goal': s, 'goal per view': pv, 'goal per step': pred.last_goal_cost_per_step}


def _frame_cost(pred, ctx, actions, goal_image, scorer):
    s = pred.score_frames(ctx, {'actions': actions}, scorer, finalweight=FINALWEIGHT)
    return {'frames': s, 'frames per step': pred.last_frame_cost_per_step}


COSTS = (_pixel_cost, _goal_cost, _frame_cost)


def _three_costs(*args):
    """Every array the three costs return or leave behind, by name."""
    out = {}
    for cost in COSTS:
        out.update(cost(*args))
    return out


@pytest.fixture(scope='module')
def single():
    """One unchunked engine, its scorer, the inputs, and its three costs on the first m actions for every m the tests use."""
    ctx, actions, goal_image = _inputs()
    pred = HipVPredEvaluation('', _hp()).restore()
    scorer = _scorer(pred.device)
    want = {m: _three_costs(pred, ctx, actions[:m], goal_image, scorer) for m in (6, 5, 2)}
    for m, arrays in want.items():
        assert arrays['score'].shape == (m,) and arrays['goal per step'].shape == (m, 1, T)
        assert arrays['frames per step'].shape == (m, T)
        for a in arrays.values():
            assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and np.isfinite(a).all()
    return ctx, actions, goal_image, scorer, want


def _assert_same(got, want):
    for name in want:
        assert got[name].dtype == np.float64 and got[name].flags['C_CONTIGUOUS'], name
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def test_an_empty_lane_share_in_every_cost(single):
    ctx, actions, goal_image, scorer, want = single
    lanes = HipVPredEvaluation('', _hp(oversubscribe_gpus=1), n_gpus=3, first_gpu=0).restore()
    assert len(lanes._lanes) == 3
    last = lanes._lanes[2]
    device = torch.cuda.current_device()
    for cost in COSTS:
        full = cost(lanes, ctx, actions[:6], goal_image, scorer)    # every lane holds something: [0, 2), [2, 4), [4, 6)
        assert (last._last_lo, last._last_M) == (4, 2), cost.__name__
        _assert_same(full, {k: want[6][k] for k in full})
        few = cost(lanes, ctx, actions[:2], goal_image, scorer)     # [0, 1), [1, 2) and nothing for the last lane
        assert (last._last_lo, last._last_M) == (2, 0), cost.__name__
        _assert_same(few, {k: want[2][k] for k in few})
        assert torch.cuda.current_device() == device, cost.__name__


def test_ragged_chunks_inside_ragged_lane_shares(single):
    ctx, actions, goal_image, scorer, want = single
    lanes = HipVPredEvaluation('', _hp(oversubscribe_gpus=1, run_batch_size=2), n_gpus=2, first_gpu=0).restore()
    assert len(lanes._lanes) == 2 and lanes.run_batch_size == 2
    got = _three_costs(lanes, ctx, actions[:5], goal_image, scorer)     # shares of 3 and 2: chunks 2 + 1 and 2
    _assert_same(got, want[5])
    assert [(l._last_lo, l._last_M) for l in lanes._lanes] == [(2, 1), (3, 2)]


def test_latent_draws_advance_once_per_scoring_call():
    ctx, actions, goal_image = _inputs()
    inputs = {'actions': actions}
    nl = 2
    hp = _hp(arch='savp', n_latent=nl, latent_seed=7)
    a, b = (StochasticHipPredictor('', hp).restore() for _ in range(2))
    scorer = _scorer(a.device, rolled=M * nl)

    def drive(p):
        out, seen = [], [p._calls]
        out.extend(p.score(ctx, inputs, GOAL_PIX, finalweight=FINALWEIGHT))
        seen.append(p._calls)
        assert p._z is None
        out.extend(p.score_goal_image(ctx, inputs, goal_image, steps='weighted', finalweight=FINALWEIGHT))
        seen.append(p._calls)
        assert p._z is None
        out.append(p.score_frames(ctx, inputs, scorer, finalweight=FINALWEIGHT))
        seen.append(p._calls)
        assert p._z is None
        assert seen == [0, 1, 2, 3]
        with pytest.raises(ValueError):         # refused by validation, counted all the same
            p.score_goal_image(ctx, inputs, goal_image, steps='nope')
        assert p._calls == 4 and p._z is None
        rolled = p(ctx, inputs)                 # the materialising path draws for itself and does not count
        assert rolled['predicted_frames'].shape == (M, T, 1, H, W, 3)
        assert p._calls == 4 and p._z is None
        out.extend(p.score(ctx, inputs, GOAL_PIX, finalweight=FINALWEIGHT))     # the draws of call 4, not of call 0
        assert p._calls == 5
        return out

    first, second = drive(a), drive(b)
    for x, y in zip(first, second):
        assert np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)
    assert np.abs(first[0] - first[-2]).max() > 0       # seed + 0 and seed + 4 are different draws

    ens = EnsembleHipPredictor('', dict(hp, num_ensembles=2)).restore()
    assert all(isinstance(m, StochasticHipPredictor) for m in ens.members)
    for k in (1, 2):
        s, _ = ens.score(ctx, inputs, GOAL_PIX, finalweight=FINALWEIGHT)
        assert np.isfinite(s).all()
        assert [m._calls for m in ens.members] == [k, 0] and ens.members[0]._z is None
