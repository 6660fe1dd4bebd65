"""``BatchedPixelCostPlanner`` on the CPU: G controllers share one fake predictor whose ``score_batch`` is its own ``score`` per
problem, so every problem must get - bit for bit - the actions and the scores of every CEM iteration that its controller
gets planning alone on a predictor of its own."""
import contextlib
import io

import numpy as np
import pytest

from tests.helpers.fake_batched_predictor import make_fake_batched_predictor_class
from visual_foresight_amd.policy.cem_controllers import BatchedPixelCostPlanner, PixelCostController
from visual_foresight_amd.policy.cem_controllers.register_gtruth_controller import RegisterGtruthController
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import PhiloxGaussianCEMSampler

T, H, W, G = 6, 16, 16, 3
AG = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
DESIG = [[[4, 5]], [[8, 8]], [[11, 3]]]
GOAL = [[[12, 12]], [[2, 13]], [[5, 9]]]


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def policy(fake, seed, **over):
    pol = dict(predictor_class=fake, verbose=False, sampler=PhiloxGaussianCEMSampler, device_cem=False, nactions=3, repeat=2,
               num_samples=12, minimum_selection=3, sampler_seed=seed)      # (iterations: the default, 3)
    pol.update(over)
    return pol


def history(g, t):
    """Problem g's observations up to step t: images [t + 1, 1, H, W, 3], states [t + 1, sdim] (a prefix of one sequence)."""
    rs = np.random.RandomState(100 + g)
    images = rs.randint(0, 256, (8, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (8, 5))
    return images[:t + 1], states[:t + 1]


def request(g, t):
    images, states = history(g, t)
    return dict(t=t, i_tr=0, desig_pix=DESIG[g], goal_pix=GOAL[g], images=images, state=states)


def run_alone(g, steps, **over):
    """Problem g's controller on a predictor of its own -> [(action, {scores_itr*}) or None] per step."""
    fake = make_fake_batched_predictor_class(T, H, W)
    with quiet():
        ctrl = PixelCostController(AG, policy(fake, 5 + g, **over), 0, 1)
        ctrl.reset()
        out = []
        for t in steps:
            res = ctrl.act(**request(g, t))
            out.append((res['actions'].copy(), {k: v.copy() for k, v in res['plan_stat'].items()}))
    assert not fake.batches
    return out


def run_batched(steps_of, **over):
    fake = make_fake_batched_predictor_class(T, H, W)
    with quiet():
        planner = BatchedPixelCostPlanner(AG, [policy(fake, 5 + g, **over) for g in range(G)], 0, 1, G)
        planner.reset()
        out = [[] for _ in range(G)]
        for call in range(len(steps_of[0])):
            res = planner.act([request(g, steps_of[g][call]) for g in range(G)])
            for g in range(G):
                out[g].append((res[g]['actions'].copy(), {k: v.copy() for k, v in res[g]['plan_stat'].items()}))
    assert len(fake.instances) == 1 and fake.instances[0].hparams['run_batch_size'] == G * 12
    return out, fake


def assert_same(batched, alone):
    for (act_b, stat_b), (act_a, stat_a) in zip(batched, alone):
        np.testing.assert_array_equal(act_b, act_a)
        assert sorted(stat_b) == sorted(stat_a)
        for key in stat_a:
            np.testing.assert_array_equal(stat_b[key], stat_a[key])


@pytest.mark.parametrize('propagation', [False, True])
def test_every_problem_plans_as_its_controller_alone(propagation):
    over = {'predictor_propagation': True} if propagation else {}
    steps = [1, 2, 3]
    batched, fake = run_batched([steps] * G, **over)
    assert fake.batches == [(G, 12)] * 9            # three iterations in each of three calls, all problems in every one
    for g in range(G):
        alone = run_alone(g, steps, **over)
        assert all(sorted(s) == ['scores_itr0', 'scores_itr1', 'scores_itr2'] for _, s in alone)
        assert_same(batched[g], alone)
    # the problems are different problems
    assert not np.array_equal(batched[0][0][1]['scores_itr0'], batched[1][0][1]['scores_itr0'])


def test_a_problem_below_start_planning_takes_no_rows():
    steps_of = [[1, 2, 3], [0, 1, 2], [1, 2, 3]]       # problem 1 starts a step later: its first call does not plan
    batched, fake = run_batched(steps_of)
    assert fake.batches == [(2, 12)] * 3 + [(G, 12)] * 6
    for g in range(G):
        assert_same(batched[g], run_alone(g, steps_of[g]))
    assert not batched[1][0][0].any() and batched[1][0][1] == {}


def test_a_replan_interval_makes_a_problem_skip_a_call():
    steps_of = [[1, 2, 3], [0, 1, 2], [1, 2, 3]]       # interval 2: problems 0 and 2 plan in calls 0 and 2, problem 1 in call 1
    batched, fake = run_batched(steps_of, replan_interval=2)
    assert fake.batches == [(2, 12)] * 3 + [(1, 12)] * 3 + [(2, 12)] * 3
    for g in range(G):
        assert_same(batched[g], run_alone(g, steps_of[g], replan_interval=2))


def test_nothing_is_launched_when_nobody_plans():
    batched, fake = run_batched([[0]] * G)
    assert fake.batches == [] and all(not b[0][0].any() for b in batched)


def test_refusals():
    fake = make_fake_batched_predictor_class(T, H, W)
    with quiet():
        with pytest.raises(ValueError, match='verbose'):
            BatchedPixelCostPlanner(AG, policy(fake, 1, verbose=True), 0, 1, G)
        pol = policy(fake, 1)
        del pol['verbose']                          # the default pages
        with pytest.raises(ValueError, match='verbose'):
            BatchedPixelCostPlanner(AG, pol, 0, 1, G)
        with pytest.raises(ValueError, match='PixelCostController itself'):
            BatchedPixelCostPlanner(AG, policy(fake, 1, type=RegisterGtruthController), 0, 1, G)
        with pytest.raises(ValueError, match='device-resident CEM'):
            BatchedPixelCostPlanner(AG, policy(fake, 1, device_cem=True), 0, 1, G)
        with pytest.raises(ValueError, match='at least one problem'):
            BatchedPixelCostPlanner(AG, policy(fake, 1), 0, 1, 0)
        with pytest.raises(ValueError, match='policyparams for'):
            BatchedPixelCostPlanner(AG, [policy(fake, 1)] * 2, 0, 1, G)
        with pytest.raises(ValueError, match='differ in'):
            BatchedPixelCostPlanner(AG, [policy(fake, 1), policy(fake, 2, num_samples=14)], 0, 1, 2)

        other = make_fake_batched_predictor_class(T, H, W)
        with pytest.raises(ValueError, match="differ in 'predictor_class'"):
            BatchedPixelCostPlanner(AG, [policy(fake, 1), policy(other, 2)], 0, 1, 2)
        with pytest.raises(ValueError, match="differ in 'model_path'"):
            BatchedPixelCostPlanner(AG, [policy(fake, 1), policy(fake, 2, model_path='/elsewhere')], 0, 1, 2)

        class Refusing(fake):
            def score_batch_refusal(self):
                return 'grouped contexts drive one engine: this predictor has 2 in-process lanes (n_gpus > 1)'
        with pytest.raises(ValueError, match='lanes'):
            BatchedPixelCostPlanner(AG, policy(Refusing, 1), 0, 1, G)
        from tests.helpers.sharded_fake import make_sharded_fake_class
        with pytest.raises(ValueError, match='score_batch'):
            BatchedPixelCostPlanner(AG, policy(make_sharded_fake_class(T, H, W), 1), 0, 1, G)

        planner = BatchedPixelCostPlanner(AG, policy(fake, 1), 0, 1, G)
        planner.reset()
        with pytest.raises(ValueError, match='verbose_worker'):
            planner.act([dict(request(g, 1), verbose_worker=object()) for g in range(G)])
        with pytest.raises(ValueError, match='requests'):
            planner.act([request(0, 1)])
    # the planner left the sampler on its host form
    assert all(c._hp.device_cem is False for c in planner.controllers)
