"""Device-resident CEM for the latent-draw, ensemble and registration planners: ``cem_latents_kernel`` /
``cem_fold_latents_kernel`` of ``csrc/vf_cem.h`` against ``philox_latents`` / ``fold_latents``, the ``score*_device`` entries of
``PhiloxStochasticHipPredictor`` and ``EnsembleHipPredictor`` against the host entries fed the device's own latents, one
teacher-forced planning call of ``PixelCostController``, ``CEM_Controller_Ensemble_Vidpred`` and
``RegisterGtruthController``, and which route a controller takes."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.helpers.device_cem_cases import ulp_distance                                             # noqa: E402
from tests.helpers.flow_warper import make_flow_warper                                              # noqa: E402
from visual_foresight_amd import _lib                                                               # noqa: E402
from visual_foresight_amd.policy.cem_controllers import PixelCostController, RegisterGtruthController   # noqa: E402
from visual_foresight_amd.policy.cem_controllers.samplers import PhiloxGaussianCEMSampler          # noqa: E402
from visual_foresight_amd.policy.cem_controllers.samplers.philox_gaussian_sampler import select_elites  # noqa: E402
from visual_foresight_amd.policy.cem_controllers.variants.ensemble_vidpred import CEM_Controller_Ensemble_Vidpred  # noqa: E402
from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor          # noqa: E402
from visual_foresight_amd.video_prediction.stochastic_predictor import (                           # noqa: E402
    PhiloxStochasticHipPredictor, StochasticHipPredictor, fold_latents, philox_latents)

DEV = 'cuda:0'
MARGIN = 1e-9       # no tested value of the Gaussian twin this close to a rejection limit (tests/test_gpu_device_cem.py)


# ----------------------------------------------------------------------------- 1. the kernels against the specification
def _device_latents(seed, call, nl, T, zdim):
    lib = _lib.load_library()
    z = torch.full((nl, T, zdim), float('nan'), dtype=torch.float32, device=DEV)
    _lib.check(lib.vf_cem_latents(0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, call & 0xFFFFFFFF, nl, T, zdim,
                                  z.data_ptr(), None))
    return z


def _device_fold(actions_dev, z, width):
    lib = _lib.load_library()
    M, T = actions_dev.shape[:2]
    nl, zdim = z.shape[0], z.shape[2]
    guard = 8       # floats behind the output that must stay as they are
    buf = torch.full((M * nl * T * (width + zdim) + guard,), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.vf_cem_fold_latents(0, actions_dev.data_ptr(), z.data_ptr(), M, nl, T, width, zdim, buf.data_ptr(), None))
    host = buf.cpu().numpy()
    assert (host[-guard:] == 7.0).all()
    return host[:-guard].reshape(M * nl, T, width + zdim)


# (n_latent, T, zdim, M, width): every dimension at its minimum; 9 normals, a partial last block; one appended constant and
# rows of 13 floats (no 16-byte alignment); 52 blocks; 80 blocks, the lanes' second pass
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 3, 5, 4), (5, 15, 8, 9, 5), (3, 13, 16, 4, 4), (2, 20, 16, 3, 4)]


@pytest.mark.parametrize('nl,T,zdim,M,width', SHAPES)
def test_kernels_match_the_specification(nl, T, zdim, M, width):
    """Latents within 1 float32 ulp of ``philox_latents`` (the free steps are the device's float64 log / sin / cos, then one
    rounding); action columns, latent columns and row order of the fold bit for bit."""
    rs = np.random.RandomState(nl * 100 + T)
    actions = rs.normal(0, 0.1, (M, T, width)).astype(np.float32)
    differing = total = 0
    for seed, call in [(31, 0), (31, 2 ** 32 - 1), ((0x01234567 << 32) | 0x89ABCDEF, 5)]:
        z = _device_latents(seed, call, nl, T, zdim)
        got = z.cpu().numpy()
        want = philox_latents(seed, call, nl, T, zdim).astype(np.float32)
        ulps = ulp_distance(got, want)
        assert not np.isnan(got).any() and ulps.max() <= 1, (seed, call, int(ulps.max()))
        differing += int((ulps > 0).sum())
        total += ulps.size
        folded = _device_fold(torch.from_numpy(actions).to(DEV), z, width)
        assert folded.tobytes() == fold_latents(actions, got).tobytes()
    print('latents %s: %d of %d values differ from the specification (by one ulp)' % ((nl, T, zdim), differing, total))
    assert not np.array_equal(_device_latents(31, 0, nl, T, zdim).cpu().numpy(), _device_latents(31, 1, nl, T, zdim).cpu().numpy())
    if width % 4 == 0 and zdim % 4 == 0:       # candidates off a 16-byte boundary take the plain stores: the same rows
        shifted = torch.zeros(actions.size + 1, dtype=torch.float32, device=DEV)
        shifted[1:] = torch.from_numpy(actions.reshape(-1)).to(DEV)
        view = shifted[1:].view(M, T, width)
        assert view.data_ptr() % 16 == 4
        assert _device_fold(view, z, width).tobytes() == folded.tobytes()


def test_argument_refusals_launch_nothing():
    lib = _lib.load_library()
    z = torch.zeros((2, 3, 8), dtype=torch.float32, device=DEV)
    a = torch.zeros((4, 3, 4), dtype=torch.float32, device=DEV)
    out = torch.zeros((8, 3, 12), dtype=torch.float32, device=DEV)
    zp, ap, op = z.data_ptr(), a.data_ptr(), out.data_ptr()
    for args in [(0, 3, 8, zp), (2, 0, 8, zp), (2, 3, 0, zp), (-1, 3, 8, zp), (2, 3, 8, None), (2, 3, 8, zp + 2),
                 (2, 2 ** 20, 2 ** 11, zp)]:
        assert lib.vf_cem_latents(0, 1, 2, 3, *args, None) == -1, args
        assert b'vf_cem_latents' in lib.vf_last_error()
    assert lib.vf_cem_latents(-1, 1, 2, 3, 2, 3, 8, zp, None) == -1
    for args in [(ap, zp, 0, 2, 3, 4, 8, op), (ap, zp, 4, 0, 3, 4, 8, op), (ap, zp, 4, 2, 0, 4, 8, op), (ap, zp, 4, 2, 3, 0, 8, op),
                 (ap, zp, 4, 2, 3, 4, 0, op), (None, zp, 4, 2, 3, 4, 8, op), (ap, None, 4, 2, 3, 4, 8, op),
                 (ap, zp, 4, 2, 3, 4, 8, None), (ap + 1, zp, 4, 2, 3, 4, 8, op), (ap, zp, 2 ** 20, 2 ** 11, 3, 4, 8, op),
                 (ap, zp, 2 ** 31 - 1, 2, 3, 4, 8, op), (ap, zp, 4, 2, 2 ** 28, 4, 4, op)]:
        assert lib.vf_cem_fold_latents(0, *args, None) == -1, args
        assert b'vf_cem_fold_latents' in lib.vf_last_error()
    assert lib.vf_cem_fold_latents(-1, ap, zp, 4, 2, 3, 4, 8, op, None) == -1
    torch.cuda.synchronize()
    assert not out.any() and not z.any()


# ----------------------------------------------------------------------------- 2. the device scoring entries
H = W = 32
T = 3
# (run_batch_size counts actions: the engine holds run_batch_size * n_latent = 4 sequences, two actions per chunk)
HP = dict(designated_pixel_count=1, run_batch_size=2, adim=4, sdim=5, image_height=H, image_width=W, sequence_length=T + 2,
          n_latent=2, latent_seed=(5 << 32) | 9)
GOAL = [[8, 20]]


def _context():
    rs = np.random.RandomState(1)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.uniform(0, 1, (2, 5)),
           'context_pixel_distributions': np.zeros((2, 1, H, W, 1), np.float32)}
    ctx['context_pixel_distributions'][:, 0, 16, 12, 0] = 1
    return ctx


@contextlib.contextmanager
def _teacher_latents(member, z_dev):
    """The host entries of ``member`` draw the latents ``z_dev`` (a device call's own) instead of the stream's."""
    z = z_dev.cpu().numpy().astype(np.float64)
    member.draw_latents = lambda T_: z
    try:
        yield
    finally:
        del member.draw_latents


@pytest.fixture(scope='module')
def stochastic():
    pred = PhiloxStochasticHipPredictor('', dict(HP), n_gpus=1, first_gpu=0).restore()
    assert pred.score_device_refusal() is None and pred.frame_score_device_refusal() is None
    assert pred.cfg.adim == 12 and pred._adim_in() == 4 and pred.run_batch_size == 4 and pred.n_draws == 2
    return pred


def test_device_entries_are_the_host_entries_fed_the_same_latents(stochastic):
    """Scores and rows bit for bit on M = 1, 2, 3 with two actions per chunk: one ragged chunk, a full chunk, a chunk edge.
    Every device call consumes one call number and draws the latents of that number."""
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    pred, ctx = stochastic, _context()
    classifier = HipFrameScorer('', dict(image_height=H, image_width=W, ncam=1, max_frames=4 * T, seed=3, bias_scale=0.2,
                                         head='classifier'), pred.device).restore()
    goal_image = np.random.RandomState(2).uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    for M in (1, 2, 3):
        actions = np.random.RandomState(M).normal(0, 0.1, (M, T, 4)).astype(np.float32)
        dev = torch.from_numpy(actions).to(pred.device)
        call = pred._calls
        got = pred.score_device(ctx, dev, GOAL, finalweight=7.)
        assert pred._calls == call + 1 and got.is_cuda and got.dtype == torch.float64 and got.shape == (M,)
        z = pred.last_latents_dev
        assert z.shape == (2, T, 8) and z.dtype == torch.float32
        want_z = philox_latents(HP['latent_seed'], call, 2, T, 8).astype(np.float32)
        assert ulp_distance(z.cpu().numpy(), want_z).max() <= 1
        seqs = pred._last_prepared[1]
        assert seqs.cpu().numpy().tobytes() == fold_latents(actions, z.cpu().numpy()).tobytes()
        per_task = pred.last_per_task_dev.cpu().numpy()
        with _teacher_latents(pred, z):
            s, pt = pred.score(ctx, {'actions': actions}, GOAL, finalweight=7.)
        assert pred._calls == call + 2
        np.testing.assert_array_equal(got.cpu().numpy(), s)
        np.testing.assert_array_equal(per_task, pt)
        assert len(np.unique(s)) == M and pred._last_M == (M if M <= 2 else 1)

        got = pred.score_goal_image_device(ctx, dev, goal_image, steps='weighted', finalweight=4.)
        z, rows = pred.last_latents_dev, pred.last_goal_rows_dev.cpu().numpy()
        with _teacher_latents(pred, z):
            s, pv = pred.score_goal_image(ctx, {'actions': actions}, goal_image, steps='weighted', finalweight=4.)
        np.testing.assert_array_equal(got.cpu().numpy(), s)
        for a, b in zip(pred.split_goal_rows(rows), (s, pv, pred.last_goal_cost_per_step)):
            np.testing.assert_array_equal(a, b)

        got = pred.score_frames_device(ctx, dev, classifier, finalweight=50.)
        z, rows = pred.last_latents_dev, pred.last_frame_rows_dev.cpu().numpy()
        with _teacher_latents(pred, z):
            s = pred.score_frames(ctx, {'actions': actions}, classifier, finalweight=50.)
        np.testing.assert_array_equal(got.cpu().numpy(), s)
        np.testing.assert_array_equal(rows[:, 0], s)
        np.testing.assert_array_equal(rows[:, 1:], pred.last_frame_cost_per_step)
        assert pred._calls == call + 6
    # the same argument checks: the caller's width, not the engine's
    with pytest.raises(ValueError, match=r'\[M, 3, 4\]'):
        pred.score_device(ctx, torch.zeros((2, T, 12), dtype=torch.float32, device=pred.device), GOAL)
    with pytest.raises(ValueError):
        pred.score_device(ctx, torch.from_numpy(actions), GOAL)            # a host tensor
    assert pred.device_status() == 0


def test_propagation_fetch_after_a_device_call(stochastic):
    """A resident action (2: the last chunk) and one that is rolled again from the folded device sequences (0)."""
    pred, ctx = stochastic, _context()
    actions = np.random.RandomState(7).normal(0, 0.1, (3, T, 4)).astype(np.float32)
    pred.score_device(ctx, torch.from_numpy(actions).to(pred.device), GOAL)
    z = pred.last_latents_dev
    assert (pred._last_lo, pred._last_M) == (2, 1)
    device = [pred.fetch_pixel_distributions(i) for i in (2, 0)]
    with _teacher_latents(pred, z):
        pred.score(ctx, {'actions': actions}, GOAL)
    for i, d in zip((2, 0), device):
        assert d.shape == (T, 1, H, W, 1) and d.any()
        np.testing.assert_array_equal(d, pred.fetch_pixel_distributions(i))
    assert not np.array_equal(device[0], device[1])


@pytest.mark.parametrize('arch', ['cdna', 'savp'])
def test_ensemble_score_device_is_score_without_the_gather(arch):
    """E = 2, M = 5 on chunks of 4 (cdna) or 2 actions (savp, two Philox draws): the whole rows bit for bit, and the
    propagation fetch."""
    hp = dict(HP, num_ensembles=2, lambda_variance=0.7)
    if arch == 'cdna':
        del hp['n_latent'], hp['latent_seed']
        hp['run_batch_size'] = 4
    else:
        hp.update(arch='savp', philox_latents=True)
    ens = EnsembleHipPredictor('', hp).restore()
    assert isinstance(ens.members[0], PhiloxStochasticHipPredictor) == (arch == 'savp')
    assert ens.score_device_refusal() is None and ens._adim_in() == 4
    ctx = _context()
    M = 5
    actions = np.random.RandomState(3).normal(0, 0.1, (M, T, 4)).astype(np.float32)
    dev = torch.from_numpy(actions).to(ens.device)
    m0 = ens.members[0]
    for first_view in (False, True):
        got = ens.score_device(ctx, dev, GOAL, finalweight=7., only_take_first_view=first_view)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (M,)
        rows = ens.last_cost_rows_dev.cpu().numpy()
        assert rows.shape == (M, 2 + T)
        fetched = [ens.fetch_pixel_distributions(i) for i in (4, 1)]
        with _teacher_latents(m0, m0.last_latents_dev) if arch == 'savp' else contextlib.nullcontext():
            s, pt = ens.score(ctx, {'actions': actions}, GOAL, finalweight=7., only_take_first_view=first_view)
        np.testing.assert_array_equal(got.cpu().numpy(), s)
        _, rows_pt, rows_cps = ens.split_cost_rows(rows)
        np.testing.assert_array_equal(rows_pt, pt)
        np.testing.assert_array_equal(rows_cps, ens.last_cost_per_step)
        assert ens.last_cost_per_step.shape == (M, 1, T) and len(np.unique(s)) == M
        for i, d in zip((4, 1), fetched):
            np.testing.assert_array_equal(d, ens.fetch_pixel_distributions(i))
    if arch == 'savp':
        assert m0._calls == 4 and all(m._calls == 0 for m in ens.members[1:])      # member 0 draws once for all
    assert ens.device_status() == 0


# ----------------------------------------------------------------------------- 3. planning calls
AG = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
POLICY = {'sampler': PhiloxGaussianCEMSampler, 'nactions': T, 'repeat': 1, 'num_samples': 8, 'iterations': 2,
          'minimum_selection': 3, 'vpred_batch_size': 4, 'verbose': False, 'sampler_seed': 21}
M_PLAN, K_PLAN, N_ITER = 8, 3, 2


class _Downloads(object):
    """Counts ``Tensor.cpu`` calls; ``at_finish`` is the count when ``_device_cem_finish`` was entered (what follows is the
    host route's own work: the propagation fetch)."""
    def __init__(self, monkeypatch, ctrl):
        self.n, self.at_finish, self.excluded = 0, None, 0
        inner_cpu = torch.Tensor.cpu
        counter = self

        def cpu(tensor, *args, **kwargs):
            counter.n += 1
            return inner_cpu(tensor, *args, **kwargs)
        monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
        inner_finish = ctrl._device_cem_finish

        def finish(*args, **kwargs):
            counter.at_finish = counter.n
            return inner_finish(*args, **kwargs)
        ctrl._device_cem_finish = finish


def _record(pred, latents_of=None):
    """Wrap ``pred.score_device``: the contexts it saw, its keyword arguments and (device tensors) the latents it drew."""
    seen, inner = [], pred.score_device

    def recording(context, actions_dev, **kw):
        out = inner(context, actions_dev, **kw)
        seen.append(dict(context={k: np.array(v) for k, v in context.items()}, kw=kw,
                         latents=None if latents_of is None else latents_of.last_latents_dev))
        return out
    pred.score_device = recording
    return seen


def _teacher_forced(ctrl, out, state, extra_keys=()):
    """The sampler's twin replayed on the device's own scores and float32 candidates: candidates within 1 ulp, the elites of
    every iteration, ``_best_actions``, the executed action and the keys of ``plan_stat``."""
    hp = ctrl._hp
    with contextlib.redirect_stdout(io.StringIO()):
        twin = PhiloxGaussianCEMSampler(hp, 4, 5)
        twin.key = ctrl._sampler.key
        proposed = twin.sample_initial_actions(1, M_PLAN, state)
    assert len(ctrl.device_candidates) == N_ITER
    for itr in range(N_ITER):
        device = ctrl.device_candidates[itr]
        assert device.shape == proposed.shape == (M_PLAN, T, 4) and device.dtype == np.float32
        assert twin.last_margin > MARGIN
        assert ulp_distance(device, proposed.astype(np.float32)).max() <= 1, itr
        scores = out['plan_stat']['scores_itr%d' % itr]
        assert scores.shape == (M_PLAN,) and scores.dtype == np.float64 and not np.isnan(scores).any()
        elites = select_elites(scores, K_PLAN)
        np.testing.assert_array_equal(ctrl.device_elite_indices[itr], elites)
        if itr + 1 < N_ITER:
            proposed = twin.sample_next_actions(M_PLAN, device[elites].astype(np.float64), scores[elites])
    assert sorted(out['plan_stat']) == sorted(['scores_itr%d' % i for i in range(N_ITER)] + list(extra_keys))
    np.testing.assert_array_equal(ctrl._best_indices, elites)
    np.testing.assert_array_equal(ctrl._best_actions, device[elites].astype(np.float64))
    np.testing.assert_array_equal(out['actions'], device[elites[0], 0].astype(np.float64))
    assert ctrl._sampler._call == twin._call == N_ITER
    assert ctrl.predictor.device_status() == 0


def _pixel_plan(ctrl, monkeypatch, latents_of=None):
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    ctrl.keep_device_candidates = True
    seen = _record(ctrl.predictor, latents_of)
    downloads = _Downloads(monkeypatch, ctrl)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, desig_pix=[[16, 12]], goal_pix=GOAL, images=frames[:1], state=states[:1])
        before = downloads.n
        out = ctrl.act(t=1, i_tr=0, desig_pix=[[16, 12]], goal_pix=GOAL, images=frames, state=states)
    monkeypatch.undo()
    del ctrl.predictor.score_device
    assert len(seen) == N_ITER and type(ctrl._device_cem).__name__ == 'DeviceCEM'      # the device route was taken
    assert downloads.at_finish - before == 1                                           # the one download of the call
    return out, seen, states[-1]


def test_stochastic_planning_call_is_the_teacher_forced_twin(monkeypatch):
    cls = PhiloxStochasticHipPredictor.with_options(n_latent=2, latent_seed=21)     # (the sampler's seed: other counters)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = PixelCostController(dict(AG), dict(POLICY, predictor_class=cls, predictor_propagation=True,
                                                  vpred_batch_size=2), 0, 1)
    pred = ctrl.predictor
    assert isinstance(pred, PhiloxStochasticHipPredictor) and pred.run_batch_size == 4 and pred.n_draws == 2
    out, seen, state = _pixel_plan(ctrl, monkeypatch, latents_of=pred)
    _teacher_forced(ctrl, out, state)
    assert pred._calls == N_ITER
    propagated = np.array(ctrl._chosen_distrib)
    for itr in range(N_ITER):       # the host route on the same candidates and latents
        want_z = philox_latents(21, itr, 2, T, 8).astype(np.float32)
        assert ulp_distance(seen[itr]['latents'].cpu().numpy(), want_z).max() <= 1
        with _teacher_latents(pred, seen[itr]['latents']):
            host, _ = pred.score(seen[itr]['context'], {'actions': ctrl.device_candidates[itr]}, GOAL,
                                 finalweight=ctrl._hp.finalweight)
        np.testing.assert_array_equal(host, out['plan_stat']['scores_itr%d' % itr])
    np.testing.assert_array_equal(propagated, pred.fetch_pixel_distributions(int(ctrl._best_indices[0])))
    assert propagated.shape == (T, 1, H, W, 1) and propagated.any()


@pytest.mark.parametrize('arch', ['cdna', 'savp'])
def test_ensemble_planning_call_is_the_teacher_forced_twin(monkeypatch, arch):
    options, pol = dict(num_ensembles=2, lambda_variance=0.7), dict(POLICY, predictor_propagation=True)
    if arch == 'savp':
        pol['vpred_batch_size'] = 2
        options.update(arch='savp', n_latent=2, philox_latents=True, latent_seed=21)
    cls = EnsembleHipPredictor.with_options(**options)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = CEM_Controller_Ensemble_Vidpred(dict(AG), dict(pol, predictor_class=cls), 0, 1)
    assert ctrl.predictor.run_batch_size == 4
    pred = ctrl.predictor
    m0 = pred.members[0]
    out, seen, state = _pixel_plan(ctrl, monkeypatch, latents_of=m0 if arch == 'savp' else None)
    _teacher_forced(ctrl, out, state)
    device_cps, propagated = ctrl.cost_perstep.copy(), np.array(ctrl._chosen_distrib)
    assert device_cps.shape == (M_PLAN, 1, 1, T)
    for itr in range(N_ITER):
        with _teacher_latents(m0, seen[itr]['latents']) if arch == 'savp' else contextlib.nullcontext():
            host, _ = pred.score(seen[itr]['context'], {'actions': ctrl.device_candidates[itr]}, GOAL,
                                 finalweight=ctrl._hp.finalweight)
        np.testing.assert_array_equal(host, out['plan_stat']['scores_itr%d' % itr])
    np.testing.assert_array_equal(device_cps.reshape(M_PLAN, 1, T), pred.last_cost_per_step)
    np.testing.assert_array_equal(propagated, pred.fetch_pixel_distributions(int(ctrl._best_indices[0])))
    assert propagated.shape == (T, 1, H, W, 1) and propagated.any()


def _registration_inputs(Hc):
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (2, 2, Hc, Hc, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal_image = rs.uniform(0, 1, (1, 2, Hc, Hc, 3)).astype(np.float32)
    return frames, states, goal_image


def _registration_controller(cls, half, **over):
    Hc = 64
    ag = {'adim': 4, 'sdim': 5, 'image_height': Hc, 'image_width': Hc, 'ncam': 2}
    if half:
        ag.update(model_image_height=Hc // 2, model_image_width=Hc // 2)
    pol = dict(POLICY, designated_pixel_count=2, registration_warper=make_flow_warper(), trade_off_reg=True,
               register_region=True, **over)
    with contextlib.redirect_stdout(io.StringIO()):
        return cls(ag, pol, 0, 1)


def _registration_plan(ctrl, half):
    frames, states, goal_image = _registration_inputs(64)
    scale = 2 if half else 1
    kw = dict(goal_image=goal_image, i_tr=0, desig_pix=[[20 // scale, 30 // scale], [40 // scale, 12 // scale]],
              goal_pix=[[10 // scale, 50 // scale], [33 // scale, 33 // scale]])
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, images=frames[:1], state=states[:1], **kw)
        return ctrl.act(t=1, images=frames, state=states, **kw), states[-1]


@pytest.mark.parametrize('half', [False, True])
def test_registration_planning_call_is_the_teacher_forced_twin(monkeypatch, half):
    """64 x 64, two views, start and goal registration with the trade-off applied; once with the model at 32 x 32."""
    ctrl = _registration_controller(RegisterGtruthController, half)
    pred = ctrl.predictor
    ctrl.keep_device_candidates = True
    seen = _record(pred)
    registered, inner_register = [], pred.register
    downloads = _Downloads(monkeypatch, ctrl)

    def register(*args, **kwargs):      # (its downloads are the one extra synchronisation, before the first rollout)
        before = downloads.n
        result = inner_register(*args, **kwargs)
        downloads.excluded += downloads.n - before
        registered.append(len(seen))
        return result
    pred.register = register
    out, state = _registration_plan(ctrl, half)
    monkeypatch.undo()
    del pred.score_device, pred.register
    assert len(seen) == N_ITER and type(ctrl._device_cem).__name__ == 'DeviceCEM'
    assert registered == [0, 0]                                    # both registrations before the first rollout
    assert downloads.at_finish - downloads.excluded == 1           # and one download
    _teacher_forced(ctrl, out, state, extra_keys=('tradeoff', 'warperrs'))
    size = 32 if half else 64
    assert (pred.cfg.height, pred.camera_size) == (size, (64, 64) if half else None)
    tradeoff = out['plan_stat']['tradeoff']
    assert tradeoff.shape == (2, 2) and abs(tradeoff.sum() - 1.0) < 1e-6
    for itr in range(N_ITER):       # the host entry on the same candidates: the tracked pixels and the weights reached the rollout
        np.testing.assert_array_equal(seen[itr]['kw']['task_weights'], tradeoff)
        host, _ = pred.score(seen[itr]['context'], {'actions': ctrl.device_candidates[itr]}, ctrl._goal_pix,
                             finalweight=ctrl._hp.finalweight, task_weights=tradeoff)
        np.testing.assert_array_equal(host, out['plan_stat']['scores_itr%d' % itr])
    # the host route registers the same frame: the same tracked pixels, weights and errors
    twin = _registration_controller(RegisterGtruthController, half, device_cem=False)
    want, _ = _registration_plan(twin, half)
    assert getattr(twin, '_device_cem', None) is None
    np.testing.assert_array_equal(ctrl._desig_pix, twin._desig_pix)
    for key in ('tradeoff', 'warperrs'):
        np.testing.assert_array_equal(out['plan_stat'][key], want['plan_stat'][key])
    on = seen[0]['context']['context_pixel_distributions']
    assert on.shape == (2, 2, size, size, 2) and on.sum() == 8.0


# ----------------------------------------------------------------------------- 4. refusals
class _Lanes(PhiloxStochasticHipPredictor):
    options = dict(n_latent=2)

    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        super(_Lanes, self).__init__(model_path, dict(hparams, oversubscribe_gpus=1), n_gpus=2, first_gpu=first_gpu)


def _overridden(cls):
    class Overridden(cls):
        def evaluate_rollouts(self, actions, cem_itr):
            return super(Overridden, self).evaluate_rollouts(actions, cem_itr)
    return Overridden


def _host_route(ctrl, plan):
    ctrl.predictor.score_device = None                  # (would raise if the device route were taken)
    out = plan(ctrl)
    assert getattr(ctrl, '_device_cem', None) is None and ctrl._sampler._call == N_ITER
    assert isinstance(ctrl._sampler, PhiloxGaussianCEMSampler)
    assert out['actions'].shape == (4,) and np.isfinite(out['actions']).all()
    for itr in range(N_ITER):
        assert np.isfinite(out['plan_stat']['scores_itr%d' % itr]).all()
    np.testing.assert_array_equal(ctrl._best_indices, select_elites(out['plan_stat']['scores_itr%d' % (N_ITER - 1)], K_PLAN))
    return out


def _plain_plan(ctrl):
    rs = np.random.RandomState(1)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.uniform(0, 1, (2, 5))
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.reset()
        ctrl.act(t=0, i_tr=0, desig_pix=[[16, 12]], goal_pix=GOAL, images=frames[:1], state=states[:1])
        return ctrl.act(t=1, i_tr=0, desig_pix=[[16, 12]], goal_pix=GOAL, images=frames, state=states)


def test_every_refusal_plans_on_the_host_route_with_the_same_sampler():
    with contextlib.redirect_stdout(io.StringIO()):
        lanes = PixelCostController(dict(AG), dict(POLICY, predictor_class=_Lanes), 0, 1)
    assert 'lanes' in lanes.predictor.score_device_refusal() and 'lanes' in lanes.predictor.frame_score_device_refusal()
    with pytest.raises(ValueError, match='lanes'):
        lanes.predictor.score_device({}, torch.zeros((2, T, 4), device=DEV), GOAL)
    _host_route(lanes, _plain_plan)
    del lanes

    random_state = EnsembleHipPredictor.with_options(num_ensembles=2, arch='savp', n_latent=2)
    with contextlib.redirect_stdout(io.StringIO()):
        ens = CEM_Controller_Ensemble_Vidpred(dict(AG), dict(POLICY, predictor_class=random_state), 0, 1)
    assert type(ens.predictor.members[0]) is StochasticHipPredictor
    assert 'the ensemble prepares its sequences on the host' in ens.predictor.score_device_refusal()
    with pytest.raises(ValueError, match='prepares its sequences on the host'):
        ens.predictor.score_device({}, torch.zeros((2, T, 4), device=DEV), GOAL)
    _host_route(ens, _plain_plan)
    assert ens.cost_perstep.shape == (M_PLAN, 1, 1, T)
    del ens

    philox = EnsembleHipPredictor.with_options(num_ensembles=2)
    with contextlib.redirect_stdout(io.StringIO()):
        again = _overridden(CEM_Controller_Ensemble_Vidpred)(dict(AG), dict(POLICY, predictor_class=philox), 0, 1)
    assert again.predictor.score_device_refusal() is None
    _host_route(again, _plain_plan)
    del again

    def registration_plan(ctrl):
        return _registration_plan(ctrl, False)[0]
    _host_route(_registration_controller(RegisterGtruthController, False, registration_on_device=False), registration_plan)
    _host_route(_registration_controller(_overridden(RegisterGtruthController), False), registration_plan)
