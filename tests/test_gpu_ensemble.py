"""Ensemble planning on the GPU: ``vf_ensemble_scores`` / ``EnsembleHipPredictor`` / ``CEM_Controller_Ensemble_Vidpred``.

* E = 1 (any lambda) and E = 2 identical members score bit-identically to the member's own ``vf_rollout``;
* distinct members: device scores, per-task rows and ``cost_per_step`` against the host restatement of the reference's
  ``ensemble_vidpred.py:32-61`` applied to every member's exported distributions;
* one CEM planning call picks the same elites as an oracle-driven ensemble; a large lambda changes the elite set;
* refusals, ``torch.distributed`` sharding and ``predictor_propagation``.
"""
import contextlib
import ctypes
import io
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                                           # noqa: E402
from tests.helpers.oracle_ensemble import make_oracle_ensemble_class                    # noqa: E402
from visual_foresight_amd import _lib                                                   # noqa: E402
from visual_foresight_amd.policy.cem_controllers.variants.ensemble_vidpred import (    # noqa: E402
    CEM_Controller_Ensemble_Vidpred, ensemble_expected_distance)
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights    # noqa: E402
from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor   # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation     # noqa: E402
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig                  # noqa: E402
from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config               # noqa: E402
from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, 'tests', 'helpers', 'ensemble_rank_worker.py')
ZDIM = 8


def _setup(arch, H, W, T, M, nd=1, ncam=1, n_latent=0):
    """Predictor hparams, a weight factory (seed) -> weights, a context, actions and goal pixels."""
    hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, ncam=ncam)
    if arch == 'cdna':
        cfg = CdnaConfig(height=H, width=W, adim=4, sdim=5, ndesig=nd, sequence_length=T + 2)
    else:
        hp.update(arch=arch, n_latent=n_latent, zdim=ZDIM, latent_seed=7)
        if arch == 'savp':
            cfg = SavpConfig(height=H, width=W, adim=4 + ZDIM, sdim=5, ndesig=nd, sequence_length=T + 2)
        else:
            cfg = Savp3Config(height=H, width=W, adim=4 + ZDIM, sdim=5, ndesig=nd, sequence_length=T + 2, zdim=ZDIM)

    def weights(seed):
        ws = [CdnaWeights.random(cfg, seed=seed + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
        return ws if ncam > 1 else ws[0]

    rs = np.random.RandomState(11)
    desig = rs.randint(4, min(H, W) - 4, (ncam, nd, 2))
    ctx = {'context_frames': rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib(desig.tolist(), 2, ncam, H, W, nd)}
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, min(H, W), (ncam, nd, 2))
    return hp, weights, ctx, actions, goal


def _export_all(member, B):
    """Normalised distributions of every rolled sequence of the member's last rollout [B, T, ncam, H, W, nd]."""
    c = member.cfg
    T = member.sequence_length - member.n_context
    with torch.cuda.device(member.device):
        out = torch.empty((B, T, member.n_cam, c.height, c.width, c.ndesig), dtype=torch.float32, device=member.device)
        _lib.check(member._libh.vf_export(member._handle, 0, B, None, out.data_ptr(), None, member._stream()))
        return out.cpu().numpy()


def _host_ensemble(dist, goal, lam, fw, n_draws):
    """Host restatement on member-major distributions [E, M * n_draws, T, ncam, H, W, nd] -> scores, per_task,
    cost_per_step [M, ncam*nd, T] (draw-averaged, as the device reports it)."""
    E, B, T, ncam, H, W, nd = dist.shape
    M = B // n_draws
    d = dist.astype(np.float64).reshape(E, M, n_draws, T, ncam, H, W, nd)
    per_task = np.zeros((M, ncam * nd))
    cps = np.zeros((M, ncam * nd, T))
    for v in range(ncam):
        for p in range(nd):
            r = np.arange(H, dtype=np.float64)[:, None] - goal[v, p, 0]
            c = np.arange(W, dtype=np.float64)[None, :] - goal[v, p, 1]
            grid = np.sqrt(r * r + c * c)
            for j in range(n_draws):
                s, step = ensemble_expected_distance(d[:, :, j, :, v, :, :, p], grid, lam, fw)
                per_task[:, v * nd + p] += s / n_draws
                cps[:, v * nd + p] += step / n_draws
    return per_task.mean(axis=1), per_task, cps


# ---------------------------------------------------------------------------------------- 1. exactness
@pytest.mark.parametrize('arch,H,W,T,M,n_latent', [('cdna', 64, 64, 4, 32, 0), ('savp', 32, 32, 3, 8, 3)])
def test_single_and_identical_members_are_bit_identical(arch, H, W, T, M, n_latent):
    hp, weights, ctx, actions, goal = _setup(arch, H, W, T, M, n_latent=n_latent)
    w = weights(3)
    single = (StochasticHipPredictor if n_latent else HipVPredEvaluation)('', hp).restore(w)
    want_s, want_pt = single.score(ctx, {'actions': actions}, goal, finalweight=7.)
    for E, lam in [(1, 0.0), (1, 0.7), (2, 0.0), (2, 0.7)]:
        ens = EnsembleHipPredictor('', dict(hp, num_ensembles=E, lambda_variance=lam)).restore([w] * E)
        assert isinstance(ens.members[0], StochasticHipPredictor) == bool(n_latent)
        s, pt = ens.score(ctx, {'actions': actions}, goal, finalweight=7.)
        np.testing.assert_array_equal(s, want_s)
        np.testing.assert_array_equal(pt, want_pt)
        assert ens.last_cost_per_step.shape == (M, 1, T)


# ---------------------------------------------------------------------------------------- 2. device vs host
@pytest.mark.parametrize('arch,H,W,T,M,nd,ncam,n_latent', [('cdna', 48, 64, 13, 12, 2, 2, 0),
                                                          ('savp3', 64, 64, 3, 4, 1, 1, 2)])
def test_device_matches_host_restatement(arch, H, W, T, M, nd, ncam, n_latent):
    hp, weights, ctx, actions, goal = _setup(arch, H, W, T, M, nd=nd, ncam=ncam, n_latent=n_latent)
    E, lam, fw = 3, 0.75, 10.
    ens = EnsembleHipPredictor('', dict(hp, num_ensembles=E, lambda_variance=lam))
    ens.restore([weights(100 * m + 1) for m in range(E)])
    s, pt = ens.score(ctx, {'actions': actions}, goal, finalweight=fw)
    nl = max(n_latent, 1)
    dist = np.stack([_export_all(m, M * nl) for m in ens.members])
    want_s, want_pt, want_cps = _host_ensemble(dist, goal, lam, fw, nl)
    np.testing.assert_allclose(s, want_s, rtol=1e-6)
    np.testing.assert_allclose(pt, want_pt, rtol=1e-6)
    np.testing.assert_allclose(ens.last_cost_per_step, want_cps, rtol=1e-6)
    # the members disagree: the variance term is not zero
    lam0 = _host_ensemble(dist, goal, 0.0, fw, nl)[0]
    assert np.abs(want_s - lam0).max() > 1e-6 * np.abs(want_s).max()


# ---------------------------------------------------------------------------------------- 3. elites vs oracle
def _plan(predictor_class, ag, pol, frames, states):
    with contextlib.redirect_stdout(io.StringIO()):
        if predictor_class is not None:
            pol = dict(pol, predictor_class=predictor_class)
        ctrl = CEM_Controller_Ensemble_Vidpred(dict(ag), dict(pol), 0, 1)
        ctrl.reset()
        np.random.seed(0)
        ctrl.act(t=0, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[6, 26]], images=frames[:1], state=states[:1])
        out = ctrl.act(t=1, i_tr=0, desig_pix=[[16, 16]], goal_pix=[[6, 26]], images=frames, state=states)
    return ctrl, out


def test_planning_elites_match_oracle_ensemble():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    E, lam, H, W = 4, 0.1, 32, 32
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    pol = {'repeat': 1, 'rejection_sampling': False, 'verbose': False}       # nactions 5, num_samples 200: defaults
    factory = lambda cfg, m: CdnaWeights.random(cfg, seed=50 + m, bias_scale=0.05, ln_jitter=0.1)
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))

    class Weighted(EnsembleHipPredictor.with_options(num_ensembles=E, lambda_variance=lam)):
        def restore(self, weights=None):
            return super(Weighted, self).restore([factory(self.cfg, m) for m in range(E)])

    ora, ora_out = _plan(make_oracle_ensemble_class(factory, E), ag, pol, frames, states)
    hip, hip_out = _plan(Weighted, ag, pol, frames, states)
    for itr in range(3):
        key = 'scores_itr%d' % itr
        s_hip, s_ora = hip_out['plan_stat'][key], ora_out['plan_stat'][key]
        np.testing.assert_allclose(s_hip, s_ora, rtol=1e-5)
        gap = np.diff(np.sort(s_ora))[9]                    # margin at the K / K+1 boundary (K = 10)
        assert gap > 4 * np.abs(s_hip - s_ora).max(), 'fixture seeds give an ambiguous elite boundary'
    np.testing.assert_array_equal(hip._best_indices, ora._best_indices)
    np.testing.assert_array_equal(hip_out['actions'], ora_out['actions'])
    np.testing.assert_allclose(hip.cost_perstep, ora.cost_perstep, rtol=1e-5)
    assert hip.cost_perstep.shape == (200, 1, 1, 5)

    # the variance term acts: a large lambda picks other elites from the same candidates
    pred = hip.predictor
    rs = np.random.RandomState(4)
    ctx = {'context_frames': frames, 'context_actions': np.zeros((1, 4)), 'context_states': states,
           'context_pixel_distributions': pixel_cost.one_hot_distrib([[[16, 16]]], 2, 1, H, W, 1)}
    actions = rs.normal(0, 0.2, (200, 5, 4))
    elites = {}
    for lam_i in (0.0, 2.5):
        pred.lambda_variance = lam_i
        s, _ = pred.score(ctx, {'actions': actions}, [[[6, 26]]])
        elites[lam_i] = set(np.argsort(s)[:10].tolist())
    assert elites[0.0] != elites[2.5]


# ---------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing():
    hp, weights, ctx, actions, goal = _setup('cdna', 32, 32, 2, 8)
    a = HipVPredEvaluation('', hp).restore(weights(1))
    b = HipVPredEvaluation('', hp).restore(weights(2))
    other = HipVPredEvaluation('', dict(hp, run_batch_size=6)).restore(weights(2))
    fresh = HipVPredEvaluation('', hp).restore(weights(3))
    lib = a._libh
    out = torch.full((8,), -7.0, dtype=torch.float64, device=a.device)

    def call(*preds):
        hs = (ctypes.c_void_p * len(preds))(*[p._handle.value for p in preds])
        rc = lib.vf_ensemble_scores(hs, len(preds), ctypes.c_float(0.1), ctypes.c_float(10.), None, out.data_ptr(),
                                    None, None, a._stream())
        return rc, lib.vf_last_error().decode()

    a.score(ctx, {'actions': actions}, goal)
    other.score(ctx, {'actions': actions[:6]}, goal)
    rc, msg = call(a, other)
    assert rc == -1 and 'vf_config' in msg
    rc, msg = call(a, fresh)
    assert rc == -1 and 'not rolled' in msg
    b.score(ctx, {'actions': actions[:6]}, goal)
    rc, msg = call(a, b)
    assert rc == -1 and 'sequences' in msg
    b.score(ctx, {'actions': actions}, goal + 1)
    rc, msg = call(a, b)
    assert rc == -1 and 'goal' in msg
    torch.cuda.synchronize(a.device)
    assert (out.cpu().numpy() == -7.0).all()
    b.score(ctx, {'actions': actions}, goal)
    rc, msg = call(a, b)
    assert rc == 0
    torch.cuda.synchronize(a.device)
    assert np.isfinite(out.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------- 5. sharding
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _launch(world, out_dir):
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=REPO, OMP_NUM_THREADS='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(port), str(out_dir)], env=env)
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [pickle.load(open(os.path.join(out_dir, 'ens_rank%d_of%d.pkl' % (r, world)), 'rb')) for r in range(world)]


def test_two_ranks_match_one(tmp_path):
    single = _launch(1, tmp_path)[0]
    for res in _launch(2, tmp_path):
        for k in ('scores', 'per_task', 'cps', 'chosen'):
            np.testing.assert_array_equal(res[k], single[k])


# ---------------------------------------------------------------------------------------- 6. propagation
def test_propagation_is_the_member_mean_of_the_chosen_action():
    E, H, W = 2, 32, 32
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    pol = {'nactions': 3, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'num_samples': 20,
           'predictor_propagation': True, 'num_ensembles': E, 'lambda_variance': 0.5}
    frames = np.random.RandomState(1).randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = np.random.RandomState(2).normal(0, .1, (2, 5))
    ctrl, out = _plan(None, ag, pol, frames, states)
    pred = ctrl.predictor
    assert isinstance(pred, EnsembleHipPredictor) and pred.num_ensembles == E and pred.lambda_variance == 0.5
    best = int(out['plan_stat']['scores_itr2'].argsort()[0])
    member_d = [_export_all(m, m._last_M)[best] for m in pred.members]
    want = (sum(d.astype(np.float64) for d in member_d) / E).astype(np.float32)
    np.testing.assert_array_equal(ctrl._chosen_distrib, want)
    assert not np.array_equal(member_d[0], member_d[1])
