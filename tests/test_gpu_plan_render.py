"""Plan visualisation on the GPU: ``vf_render_plans`` / ``HipVPredEvaluation.render_plans`` / the controllers' plan page.

* the device's bytes equal ``visualizer/colormap.py`` applied to the same sequences' exported frames and distributions,
  bit for bit (both sides start from the same float32 values);
* the resident render, the re-rolled render, chunks, in-process lanes and gloo ranks give the same bytes, and a
  propagation fetch after a re-rolled render still returns what it returned before;
* one verbose planning call on the HIP predictor against the same controller on the CPU oracle with host rendering;
* refusals on a live handle, indices outside the last call.
"""
import contextlib
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

from tests.helpers.oracle_predictor import make_oracle_predictor_class                  # noqa: E402
from visual_foresight_amd import _lib                                                   # noqa: E402
from visual_foresight_amd.policy.cem_controllers import GoalImController, PixelCostController   # noqa: E402
from visual_foresight_amd.policy.cem_controllers.visualizer import colormap             # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights    # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation     # noqa: E402
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig                  # noqa: E402
from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config               # noqa: E402
from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, 'tests', 'helpers', 'plan_render_rank_worker.py')
ZDIM = 8


def _setup(arch, H, W, T, M, ncam=1, nd=1, n_latent=0, run_batch_size=None, **extra):
    """A restored predictor, a context with ``nd`` designated pixels per view, actions and goal pixels."""
    hp = dict(designated_pixel_count=nd, run_batch_size=run_batch_size or M, adim=4, sdim=5, image_height=H,
              image_width=W, sequence_length=T + 2, ncam=ncam, **extra)
    if arch == 'cdna':
        cfg = CdnaConfig(height=H, width=W, adim=4, sdim=5, ndesig=nd, sequence_length=T + 2)
    else:
        hp.update(arch=arch, n_latent=n_latent, zdim=ZDIM, latent_seed=7)
        if arch == 'savp':
            cfg = SavpConfig(height=H, width=W, adim=4 + ZDIM, sdim=5, ndesig=nd, sequence_length=T + 2)
        else:
            cfg = Savp3Config(height=H, width=W, adim=4 + ZDIM, sdim=5, ndesig=nd, sequence_length=T + 2, zdim=ZDIM)
    ws = [CdnaWeights.random(cfg, seed=3 + v, bias_scale=0.05, ln_jitter=0.1) for v in range(ncam)]
    n_gpus = 2 if extra.get('oversubscribe_gpus') else 1
    cls = StochasticHipPredictor if n_latent else HipVPredEvaluation
    pred = cls('', hp, n_gpus=n_gpus, first_gpu=0).restore(ws if ncam > 1 else ws[0])
    rs = np.random.RandomState(11)
    distrib = np.zeros((2, ncam, H, W, nd), np.float32)
    goal = np.zeros((ncam, nd, 2), np.int64)
    for v in range(ncam):
        for p in range(nd):
            distrib[:, v, rs.randint(H), rs.randint(W), p] = 1.
            goal[v, p] = rs.randint(H), rs.randint(W)
    ctx = {'context_frames': rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': distrib}
    return pred, ctx, rs.normal(0, 0.1, (M, T, 4)), goal


def _export(pred, B):
    """Frames and normalised distributions of every rolled sequence of the last rollout, as ``vf_export`` gives them."""
    c = pred.cfg
    T = pred.sequence_length - pred.n_context
    with torch.cuda.device(pred.device):
        f = torch.empty((B, T, pred.n_cam, c.height, c.width, 3), dtype=torch.float32, device=pred.device)
        d = torch.empty((B, T, pred.n_cam, c.height, c.width, c.ndesig), dtype=torch.float32, device=pred.device)
        _lib.check(pred._libh.vf_export(pred._handle, 0, B, f.data_ptr(), d.data_ptr(), None, pred._stream()))
        return f.cpu().numpy(), d.cpu().numpy()


# ---------------------------------------------------------------------------------------- 1. device = host
CASES = [('cdna', 64, 64, 3, 12, 2, 2, 0), ('cdna', 48, 64, 2, 9, 1, 4, 0), ('cdna', 32, 40, 2, 6, 1, 3, 0),
         ('cdna', 32, 32, 2, 6, 1, 1, 0), ('savp', 32, 32, 3, 5, 1, 2, 3), ('savp3', 64, 64, 2, 4, 1, 1, 2)]


@pytest.mark.parametrize('arch,H,W,T,M,ncam,nd,n_latent', CASES)
def test_device_equals_host_bit_for_bit(arch, H, W, T, M, ncam, nd, n_latent):
    nl = max(n_latent, 1)
    pred, ctx, actions, goal = _setup(arch, H, W, T, M, ncam=ncam, nd=nd, n_latent=n_latent)
    pred.score(ctx, {'actions': actions}, goal_pix=goal)
    idx = np.random.RandomState(1).permutation(M)[:max(M - 2, 1)]                # a shuffled subset
    got = pred.render_plans(idx)
    assert pred._last_M == M                                                     # rendered where it lay: nothing re-rolled
    frames, distrib = _export(pred, M * nl)
    want = colormap.render_prediction(frames[idx * nl], distrib[idx * nl])       # the first draw of every action
    K = len(idx)
    assert got['frames'].shape == (K, ncam, T, H, W, 3) and got['frames'].dtype == np.uint8
    assert got['distributions'].shape == (K, ncam, nd, T, H, W, 3) and got['distributions'].dtype == np.uint8
    np.testing.assert_array_equal(got['frames'], want['frames'])
    np.testing.assert_array_equal(got['distributions'], want['distributions'])
    assert len(np.unique(got['frames'])) > 16 and len(np.unique(got['distributions'].reshape(-1, 3), axis=0)) > 16
    # every plane reaches the top of the table (its own maximum) and another colour table goes through unchanged
    top = (got['distributions'] == colormap.VIRIDIS_U8[255]).all(axis=-1).any(axis=(-2, -1))
    assert top.all()
    lut = np.random.RandomState(2).randint(0, 256, (256, 3)).astype(np.uint8)
    other = pred.render_plans(idx[:2], lut=lut, frames=False)
    assert list(other) == ['distributions']
    np.testing.assert_array_equal(other['distributions'],
                                  colormap.render_prediction(None, distrib[idx[:2] * nl], lut)['distributions'])
    only = pred.render_plans(idx[:1], distributions=False)
    assert list(only) == ['frames']
    np.testing.assert_array_equal(only['frames'], want['frames'][:1])


# ---------------------------------------------------------------------------------------- 2. the paths agree
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
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [pickle.load(open(os.path.join(out_dir, 'render_rank%d_of%d.pkl' % (r, world)), 'rb')) for r in range(world)]


def test_resident_rerolled_chunked_and_lanes_agree():
    H, W, T, M, ncam, nd = 64, 64, 3, 24, 2, 2
    one, ctx, actions, goal = _setup('cdna', H, W, T, M, ncam=ncam, nd=nd)
    chunked = _setup('cdna', H, W, T, M, ncam=ncam, nd=nd, run_batch_size=8)[0]
    lanes = _setup('cdna', H, W, T, M, ncam=ncam, nd=nd, oversubscribe_gpus=1)[0]
    assert chunked.run_batch_size == 8 and len(lanes._lanes) == 2
    idx = np.array([20, 3, 14, 7, 23, 0, 9, 12, 16, 5])                          # spans chunks and both lanes
    scores = one.score(ctx, {'actions': actions}, goal_pix=goal)[0]
    resident = one.render_plans(idx)
    assert (one._last_lo, one._last_M) == (0, M)
    fetched = one.fetch_pixel_distributions(14)
    one._last_M = 0                                         # as if another chunk had been rolled since: forces the re-roll
    rerolled = one.render_plans(idx)
    assert one._last_M == 0
    np.testing.assert_array_equal(one.fetch_pixel_distributions(14), fetched)   # the fetch re-rolls it, same bits
    assert (one._last_lo, one._last_M) == (14, 1)
    results = [rerolled]
    for pred in (chunked, lanes):
        np.testing.assert_array_equal(pred.score(ctx, {'actions': actions}, goal_pix=goal)[0], scores)
        results.append(pred.render_plans(idx))
        np.testing.assert_array_equal(pred.fetch_pixel_distributions(14), fetched)
    assert len(idx) > chunked.run_batch_size                # more plans than one rollout holds: re-rolled in groups
    for other in results:
        np.testing.assert_array_equal(other['frames'], resident['frames'])
        np.testing.assert_array_equal(other['distributions'], resident['distributions'])
    assert len(np.unique(resident['frames'].reshape(len(idx), -1), axis=0)) == len(idx)     # the plans do differ


def test_two_ranks_match_one(tmp_path):
    single = _launch(1, tmp_path)[0]
    assert single['frames'].shape == (7, 2, 3, 32, 32, 3) and single['distributions'].shape == (7, 2, 2, 3, 32, 32, 3)
    np.testing.assert_array_equal(single['fetch_after'], single['fetch_before'])
    for res in _launch(2, tmp_path):
        for k in ('scores', 'frames', 'distributions', 'fetch_before', 'fetch_after'):
            np.testing.assert_array_equal(res[k], single[k], err_msg=k)


# ---------------------------------------------------------------------------------------- 3. closed loop
class RecordingWorker(object):
    def __init__(self):
        self.messages = []

    def put(self, message):
        self.messages.append(message)


def _weights(cfg):
    return CdnaWeights.random(cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)


class Weighted(HipVPredEvaluation):
    def restore(self, weights=None):
        return super(Weighted, self).restore(_weights(self.cfg))


def _plan(controller, predictor_class, pol, seed, **kw):
    H = W = 32
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    rs = np.random.RandomState(2)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    worker = RecordingWorker()
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = controller(dict(ag), dict(pol, predictor_class=predictor_class), 0, 1)
        ctrl.reset()
        np.random.seed(seed)
        ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1], verbose_worker=worker, **kw)
        out = ctrl.act(t=1, i_tr=0, images=frames, state=states, verbose_worker=worker, **kw)
    return ctrl, out, worker.messages


def _compare_pages(hip, ora):
    """Kinds and paths identical; the scores row to 1e-5; payload bytes within the allowances derived in the docstrings."""
    from visual_foresight_amd.policy.cem_controllers.visualizer.plan_page import parse_plan_page
    (hip_ctrl, hip_out, hip_msgs), (ora_ctrl, ora_out, ora_msgs) = hip, ora
    s_hip, s_ora = hip_out['plan_stat']['scores_itr0'], ora_out['plan_stat']['scores_itr0']
    diff = np.abs(s_hip - s_ora).max()
    gaps = np.diff(np.sort(s_ora))[:10]                     # the ORDER of the ten shown plans is compared: every gap counts
    print('max |device - oracle| %.3g, smallest oracle gap among the shown plans %.3g' % (diff, gaps.min()))
    assert gaps.min() > 4 * diff, 'fixture seeds give an ambiguous order of the shown plans'
    np.testing.assert_array_equal(hip_ctrl.visualize_indices, ora_ctrl.visualize_indices)
    assert [(m[0], m[1]) for m in hip_msgs] == [(m[0], m[1]) for m in ora_msgs]
    lut = colormap.VIRIDIS_U8.astype(np.int64)
    colour_step = int(np.abs(np.diff(lut, axis=0)).max())   # the largest step between adjacent table rows
    for got, want in zip(hip_msgs, ora_msgs):
        if got[0] == 'img':
            np.testing.assert_array_equal(got[2], want[2])
        elif got[0] == 'mov':
            a, b = got[2].astype(np.int64), want[2].astype(np.int64)
            assert a.shape == b.shape
            differing = float((a != b).mean())
            allowed = colour_step if '_desig_' in got[1] else 1
            print('%s: %.4f %% of the bytes differ, by at most %d' % (got[1], 100 * differing, np.abs(a - b).max()))
            assert np.abs(a - b).max() <= allowed, got[1]
            assert differing <= 0.01, got[1]
        else:
            c_hip, c_ora = parse_plan_page(got[2]), parse_plan_page(want[2])
            rows_hip, rows_ora = dict(c_hip['rows']), dict(c_ora['rows'])
            np.testing.assert_allclose([float(s) for s in rows_hip.pop('scores')],
                                       [float(s) for s in rows_ora.pop('scores')], rtol=1e-5)
            assert rows_hip == rows_ora and [r[0] for r in c_hip['rows']] == [r[0] for r in c_ora['rows']]
            assert {k: v for k, v in c_hip.items() if k != 'rows'} == {k: v for k, v in c_ora.items() if k != 'rows'}


BASE_POLICY = {'num_samples': 16, 'iterations': 1, 'repeat': 1, 'rejection_sampling': False, 'initial_std': 0.5,
               'initial_std_lift': 0.6}


def test_pixel_cost_page_matches_the_oracle_controller():
    """One verbose planning call (16 samples, 32 x 32, two designated pixels, T = 5): the HIP predictor renders on the
    device, the CPU oracle predictor is rendered on the host.  Seed chosen on the CPU oracles alone, before any device run:
    the smallest gap among the ten shown plans' float32-oracle scores is 2.1e-4, 127 times the float32 / float64 oracle
    difference (1.6e-6).

    Payloads are truncations of values that agree to the parity tolerances (1e-5 relative on frames and distributions):
    a frame byte may differ by 1 where ``frame * 255`` straddles an integer (1e-5 * 255 < 1); a table index by 1
    (|dq| * 256 < 0.02), hence a colour byte by at most the largest step between adjacent table rows; and at most 1 % of a
    movie's bytes may differ at all.  Counted on the CPU between the float32 and the float64 oracle for this fixture
    (seeds 0 - 3): 0 to 1e-5 of all movie bytes differ, 1.3e-4 (0.013 %) in the worst movie, never by more than 1."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    pol = dict(BASE_POLICY, designated_pixel_count=2)
    kw = dict(desig_pix=[[16, 16], [8, 20]], goal_pix=[[8, 24], [20, 6]])
    ora = _plan(PixelCostController, make_oracle_predictor_class(_weights), pol, 0, **kw)
    hip = _plan(PixelCostController, Weighted, pol, 0, **kw)
    assert hasattr(hip[0].predictor, 'render_plans') and not hasattr(ora[0].predictor, 'render_plans')
    assert ora[0].predictor.calls == 2 and len(hip[2]) == 1 + 20 + 10 + 1      # the oracle rolled the ten again for its page
    _compare_pages(hip, ora)
    np.testing.assert_array_equal(hip[1]['actions'], ora[1]['actions'])


def test_goal_image_page_matches_the_oracle_controller():
    """As above for ``GoalImController`` (rows: start, goal, predicted images, scores).  Seed 2, chosen on the CPU oracles
    alone: smallest gap among the shown plans 3.8e-6 against a float32 / float64 oracle difference of 2.9e-9; no byte of
    any movie differed between the two oracles."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    goal = np.random.RandomState(7).randint(0, 256, (32, 32, 3)).astype(np.uint8)
    ora = _plan(GoalImController, make_oracle_predictor_class(_weights), BASE_POLICY, 2, goal_image=goal)
    hip = _plan(GoalImController, Weighted, BASE_POLICY, 2, goal_image=goal)
    assert [m[0] for m in hip[2]] == ['img', 'img'] + ['mov'] * 10 + ['txt_file']
    _compare_pages(hip, ora)
    np.testing.assert_array_equal(hip[1]['actions'], ora[1]['actions'])


# ---------------------------------------------------------------------------------------- 4. refusals
def test_refusals_on_a_live_handle():
    import ctypes
    pred, ctx, actions, goal = _setup('cdna', 32, 32, 2, 8)
    lib = pred._libh
    with pytest.raises(IndexError):
        pred.render_plans([0])                                                  # no scoring call yet
    with torch.cuda.device(pred.device):
        seq = torch.zeros(16, dtype=torch.int32, device=pred.device)
        lut = torch.from_numpy(np.array(colormap.VIRIDIS_U8)).to(pred.device)
        f = torch.full((16, 1, 2, 32, 32, 3), 77, dtype=torch.uint8, device=pred.device)
        d = torch.full((16, 1, 1, 2, 32, 32, 3), 77, dtype=torch.uint8, device=pred.device)

        def call(seq_ptr, K, lut_ptr, f_ptr, d_ptr):
            rc = lib.vf_render_plans(pred._handle, seq_ptr, K, lut_ptr, f_ptr, d_ptr, pred._stream())
            return rc, lib.vf_last_error().decode()

        rc, msg = call(seq.data_ptr(), 1, lut.data_ptr(), f.data_ptr(), d.data_ptr())
        assert rc == -1 and 'not rolled' in msg
        scores = pred.score(ctx, {'actions': actions}, goal_pix=goal)[0]
        for args, word in (((None, 1, lut.data_ptr(), f.data_ptr(), d.data_ptr()), 'null'),
                           ((seq.data_ptr(), 1, lut.data_ptr(), None, None), 'both outputs'),
                           ((seq.data_ptr(), 1, None, f.data_ptr(), d.data_ptr()), 'colour table'),
                           ((seq.data_ptr(), 0, lut.data_ptr(), f.data_ptr(), d.data_ptr()), 'at least one'),
                           ((seq.data_ptr(), 9, lut.data_ptr(), f.data_ptr(), d.data_ptr()), 'max_batch')):
            rc, msg = call(*args)
            assert rc == -1 and word in msg, (args, msg)
        torch.cuda.synchronize(pred.device)
        assert (f.cpu().numpy() == 77).all() and (d.cpu().numpy() == 77).all()                  # nothing was launched
        # frames alone need no table; entries of d_seq outside the rollout are clamped into it, never followed
        wild = torch.tensor([-5, 3, 1000], dtype=torch.int32, device=pred.device)
        _lib.check(lib.vf_render_plans(pred._handle, wild.data_ptr(), 3, None, f.data_ptr(), None, pred._stream()))
        got = f[:3].cpu().numpy()
    want = pred.render_plans([0, 3, 7], distributions=False)['frames']
    np.testing.assert_array_equal(got, want)
    for bad in ([8], [-1], [0, 99]):
        with pytest.raises(IndexError):
            pred.render_plans(bad)
    for bad in ([], [1, 1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            pred.render_plans(bad)
    with pytest.raises(ValueError):
        pred.render_plans([0], frames=False, distributions=False)
    with pytest.raises(ValueError):
        pred.render_plans([0], lut=np.zeros((16, 3), np.uint8))
    np.testing.assert_array_equal(pred.score(ctx, {'actions': actions}, goal_pix=goal)[0], scores)
