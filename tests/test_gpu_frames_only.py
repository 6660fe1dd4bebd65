"""GPU: frames-only engines (``vf_config.ndesig`` 0 - ``designated_pixel_count`` 0, ``no_pix_distrib``,
``FramesOnlyHipVPredEvaluation``).

1. The frames and states of a frames-only engine are, bit for bit, those of the engine with one designated pixel built from
   the same weights: every table (arch 0 with layer_spec 0 - 3, arch 1, arch 2), every launch route, ``xcd_queues`` on and off,
   both reduced precisions, two views, one context frame, a cached context, a permuted batch.  ``assert_array_equal``: a frame
   pixel runs the same fma chain in both instances, and nothing a frame depends on reads a distribution.
2. Frames against the CPU oracles run with one dummy distribution channel, one table per compositing mode, at the bounds of
   those tables' own parity tests (``test_gpu_parity.py``, ``test_gpu_appflow.py``, ``test_gpu_dna.py``, ``test_gpu_savp.py``:
   frames 1e-5, states 1e-6).
3. Goal-image and learned costs, and the rendered frames, against the one-pixel engine: equal.
4. Every refusal of the C ABI and of the Python surface; the handle stays usable.
5. One planning call of each frame-cost controller with either predictor class: the same scores, elites, action and page.
6. The frames-only handle allocates less device memory, by at least the distribution tensors.
7. arch 3 has no frames-only heads: ``vf_create`` refuses ``ndesig`` 0 there.
"""
import contextlib
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.helpers.fake_frames_only_predictor import assert_same_messages                        # noqa: E402
from visual_foresight_amd import _lib                                                            # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights              # noqa: E402
from visual_foresight_amd.video_prediction.dna_arch import DnaConfig                             # noqa: E402
from visual_foresight_amd.video_prediction.hip_predictor import (FramesOnlyHipVPredEvaluation,   # noqa: E402
                                                                 HipVPredEvaluation)
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig, Savp2Config              # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 3

# table -> (config class, config arguments, predictor hyper-parameters, action channels)
TABLES = {
    'cdna': (CdnaConfig, {}, {}, 4),
    'public': (CdnaConfig, {'decoder': 'public'}, {'decoder': 'public'}, 4),
    'flow': (CdnaConfig, {'transformation': 'flow'}, {'transformation': 'flow'}, 4),
    'dna': (DnaConfig, {}, {'transformation': 'dna'}, 4),
    'savp': (SavpConfig, {}, {'arch': 'savp'}, 6),
    'savp2': (Savp2Config, {}, {'arch': 'savp2'}, 6),
}


def _weights(table, H, W, nc=2, seed=3):
    cls, cargs, _, adim = TABLES[table]
    cfg = cls(height=H, width=W, adim=adim, ndesig=1, n_context=nc, sequence_length=T + nc, **cargs)
    return CdnaWeights.random(cfg, seed=seed, bias_scale=0.05, ln_jitter=0.1)


def _pair(table, H, W, M, nc=2, ncam=1, **extra):
    """-> (frames-only predictor, the predictor with one designated pixel) from the same weights."""
    _, _, hp_extra, adim = TABLES[table]
    ws = [_weights(table, H, W, nc, seed=3 + v) for v in range(ncam)]
    out = []
    for nd in (0, 1):
        hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=adim, sdim=5, image_height=H, image_width=W,
                  sequence_length=T + nc, n_context=nc, ncam=ncam, **dict(hp_extra, **extra))
        out.append(HipVPredEvaluation('', hp).restore(ws if ncam > 1 else ws[0]))
    assert out[0].frames_only is True and out[1].frames_only is False
    assert out[0].cfg.ndesig == 0 and out[0].cfg.tensor_shapes() == out[1].cfg.tensor_shapes()
    return out[0], out[1], ws


def _contexts(H, W, adim, rs, nc=2, ncam=1):
    """-> (context without distributions, the same with a one-hot for the one-pixel engine)."""
    hist = nc + 1 if nc > 1 else 1
    ctx = {'context_frames': rs.randint(0, 256, (hist, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (hist - 1, adim)),
           'context_states': rs.normal(0, 0.1, (hist, 5))}
    d = np.zeros((nc, ncam, H, W, 1), np.float32)
    d[:, :, H // 3, W // 2, 0] = 1.
    return ctx, dict(ctx, context_pixel_distributions=d)


ROUTES = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1)]          # (persistent, fuse_top, xcd_queues)

IDENTITY_CASES = [
    # table, H, W, M, n_context, ncam, predictor extras
    ('cdna', 32, 32, 5, 2, 1, {}), ('cdna', 48, 64, 9, 2, 1, {}),
    ('cdna', 40, 56, 5, 2, 1, {}),                                        # a top that cannot be fused: two phases on every route
    ('cdna', 32, 32, 5, 1, 1, {}), ('cdna', 32, 32, 5, 2, 2, {}),
    ('cdna', 32, 32, 5, 2, 1, {'precision': 'bf16x6'}), ('cdna', 48, 64, 9, 2, 1, {'precision': 'bf16'}),
    ('public', 32, 32, 5, 2, 1, {}), ('public', 48, 64, 9, 2, 1, {}),
    ('flow', 32, 32, 5, 2, 1, {}), ('flow', 48, 64, 9, 2, 1, {}),
    ('dna', 32, 32, 5, 2, 1, {}), ('dna', 48, 64, 9, 2, 1, {}),
    ('savp', 32, 32, 5, 2, 1, {}), ('savp', 48, 64, 9, 2, 1, {}),
    ('savp2', 64, 64, 5, 2, 1, {}),                                       # (arch 2 needs 64 x 64)
]


@pytest.mark.parametrize('table,H,W,M,nc,ncam,extra', IDENTITY_CASES)
def test_frames_and_states_are_bit_identical_to_the_one_pixel_engine(table, H, W, M, nc, ncam, extra):
    p0, p1, _ = _pair(table, H, W, M, nc=nc, ncam=ncam, **extra)
    adim = TABLES[table][3]
    rs = np.random.RandomState(H + W + M + nc + ncam)
    ctx0, ctx1 = _contexts(H, W, adim, rs, nc=nc, ncam=ncam)
    actions = rs.normal(0, 0.1, (M, T, adim))
    perm = np.roll(np.arange(M), 1)
    want = p1(ctx1, {'actions': actions})
    assert p1.device_status() == 0
    assert np.ptp(want['predicted_frames']) > 0.1 and np.isfinite(want['predicted_frames']).all()
    assert np.abs(want['predicted_frames'][0] - want['predicted_frames'][1]).max() > 0        # the actions matter
    for persistent, fuse, xcd in ROUTES:
        p0.set_persistent(persistent)
        p0.set_fuse_top(fuse)
        p0.set_xcd_queues(xcd)
        for rep in range(2):                    # the second call finds the context (and the shared units) cached
            got = p0(ctx0, {'actions': actions})
            assert p0.device_status() == 0
            assert got['predicted_pixel_distributions'] is None
            np.testing.assert_array_equal(got['predicted_frames'], want['predicted_frames'])
            np.testing.assert_array_equal(got['predicted_states'], want['predicted_states'])
        gp = p0(ctx0, {'actions': actions[perm]})
        assert p0.device_status() == 0
        np.testing.assert_array_equal(gp['predicted_frames'], want['predicted_frames'][perm])
        np.testing.assert_array_equal(gp['predicted_states'], want['predicted_states'][perm])
        p0._ctx_key = None                      # upload the context again: the next route computes the shared units itself


def test_chunks_lanes_latent_draws_and_the_legacy_boundary():
    """Chunked batches, two in-process lanes, latent draws (``StochasticHipPredictor``) and ``predictor_func``."""
    from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor
    H = W = 32
    M = 9
    p0, p1, w = _pair('cdna', H, W, M)
    rs = np.random.RandomState(5)
    ctx0, ctx1 = _contexts(H, W, 4, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    want = p1(ctx1, {'actions': actions})
    hp = dict(designated_pixel_count=0, adim=4, sdim=5, image_height=H, image_width=W, sequence_length=T + 2)
    chunked = HipVPredEvaluation('', dict(hp, run_batch_size=4)).restore(w[0])
    lanes = HipVPredEvaluation('', dict(hp, run_batch_size=M, oversubscribe_gpus=1), n_gpus=2).restore(w[0])
    assert len(lanes._lanes) == 2 and all(l.frames_only for l in lanes._lanes)
    for other in (chunked, lanes):
        got = other(ctx0, {'actions': actions})
        assert got['predicted_pixel_distributions'] is None and other.device_status() == 0
        np.testing.assert_array_equal(got['predicted_frames'], want['predicted_frames'])
        np.testing.assert_array_equal(got['predicted_states'], want['predicted_states'])
    # the legacy boundary: gen_distrib is None, as the reference returns it without a one-hot input
    acts = np.concatenate([np.tile(ctx0['context_actions'][-1:], (M, 1, 1)), actions], axis=1)
    f, d, s = p0.predictor_func()(input_images=ctx0['context_frames'][-2:][None].astype(np.float32) / 255.,
                                  input_one_hot_images=None, input_state=ctx0['context_states'][-2:][None], input_actions=acts)
    assert d is None
    np.testing.assert_array_equal(f, want['predicted_frames'])
    np.testing.assert_array_equal(s, want['predicted_states'])
    # latent draws: the same draws, the same goal-image costs
    shp = dict(adim=4, sdim=5, image_height=H, image_width=W, sequence_length=T + 2, run_batch_size=M, n_latent=2, zdim=2,
               arch='savp')
    cfg = SavpConfig(height=H, width=W, adim=6, ndesig=1, sequence_length=T + 2)
    ws = CdnaWeights.random(cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)
    goal = rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    res = []
    for nd in (0, 1):
        sp = StochasticHipPredictor('', dict(shp, designated_pixel_count=nd)).restore(ws)
        assert sp.frames_only == (nd == 0)
        res.append(sp.score_goal_image(ctx0, {'actions': actions}, goal, steps='weighted') + (sp.last_goal_cost_per_step,))
        assert sp.device_status() == 0
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    assert len(np.unique(res[0][0])) == M


# ---------------------------------------------------------------------------------------- 2. oracle parity
def _oracle_class(table):
    if table == 'cdna':
        from oracle.cdna_predictor import OracleCdna
        return OracleCdna
    if table == 'flow':
        from tests.helpers.oracle_appflow import OracleAppflow
        return OracleAppflow
    if table == 'dna':
        from tests.helpers.oracle_dna import OracleDna
        return OracleDna
    from oracle.savp_predictor import OracleSavp, OracleSavp2
    return OracleSavp if table == 'savp' else OracleSavp2


@pytest.mark.parametrize('table,H,W,M', [('cdna', 48, 64, 5), ('flow', 48, 64, 5), ('dna', 48, 64, 5), ('savp', 32, 32, 5),
                                         ('savp2', 64, 64, 3)])
def test_frames_match_the_oracle_run_with_a_dummy_distribution(table, H, W, M):
    p0, _, ws = _pair(table, H, W, M)
    adim = TABLES[table][3]
    rs = np.random.RandomState(H + W + M)
    ctx0, ctx1 = _contexts(H, W, adim, rs)
    actions = rs.normal(0, 0.1, (M, T, adim))
    got = p0(ctx0, {'actions': actions})
    f, _, s = _oracle_class(table)(ws[0], torch.float32).rollout(
        ctx1['context_frames'], ctx1['context_actions'], ctx1['context_pixel_distributions'], ctx1['context_states'], actions)
    err_f, err_s = np.abs(got['predicted_frames'] - f).max(), np.abs(got['predicted_states'] - s).max()
    print('frames-only parity %s %dx%d: frames %.3g  states %.3g' % (table, H, W, err_f, err_s))
    assert err_f <= 1e-5
    assert err_s <= 1e-6
    assert p0.device_status() == 0


# ---------------------------------------------------------------------------------------- 3. costs
@pytest.mark.parametrize('table,H,W,M,ncam', [('cdna', 32, 32, 9, 1), ('flow', 48, 64, 5, 1), ('cdna', 32, 32, 5, 2)])
def test_frame_costs_and_rendered_frames_equal_the_one_pixel_engines(table, H, W, M, ncam):
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    p0, p1, _ = _pair(table, H, W, M, ncam=ncam)
    rs = np.random.RandomState(H + M + ncam)
    ctx0, _ = _contexts(H, W, 4, rs, ncam=ncam)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.uniform(0, 1, (ncam, H, W, 3)).astype(np.float32)
    shp = dict(image_height=H, image_width=W, ncam=ncam, max_frames=M * T, seed=4, bias_scale=0.2)
    cls_s = HipFrameScorer('', dict(shp, head='classifier'), p0.device).restore()
    emb_s = HipFrameScorer('', dict(shp, head='embedding', embed_dim=8), p0.device).restore()
    goal_enc = emb_s.embed(rs.uniform(0, 1, (1, ncam, H, W, 6)).astype(np.float32), 'goal')[0]
    idx = np.array([M - 1, 0, 2])
    for steps in ('last', 'weighted'):
        res = []
        for p in (p0, p1):
            s, pv = p.score_goal_image(ctx0, {'actions': actions}, goal, steps=steps, finalweight=7.)
            res.append((s, pv, p.last_goal_cost_per_step, p.render_plans(idx, frames=True, distributions=False)['frames']))
            assert p.device_status() == 0
        for a, b in zip(*res):
            np.testing.assert_array_equal(a, b)
        assert len(np.unique(res[0][0])) == M and res[0][3].dtype == np.uint8 and np.ptp(res[0][3]) > 0
    for scorer, enc in ((cls_s, None), (emb_s, goal_enc)):
        res = []
        for p in (p0, p1):
            s = p.score_frames(ctx0, {'actions': actions}, scorer, goal_enc=enc, finalweight=6.)
            res.append((s, p.last_frame_cost_per_step) + p.score_resident_frames(scorer, enc, 6.))
            assert p.device_status() == 0
        for a, b in zip(*res):
            np.testing.assert_array_equal(a, b)
        assert len(np.unique(res[0][0])) == M


# ---------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_handle_usable():
    H = W = 32
    M = 5
    p0, p1, w = _pair('cdna', H, W, M)
    rs = np.random.RandomState(9)
    ctx0, ctx1 = _contexts(H, W, 4, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    good = p0(ctx0, {'actions': actions})
    lib, h = p0._libh, p0._handle

    def refused(rc):
        msg = lib.vf_last_error().decode()
        assert rc == -1 and 'frames-only' in msg, (rc, msg)

    def still_good():
        assert p0.device_status() == 0
        again = p0(ctx0, {'actions': actions})
        np.testing.assert_array_equal(again['predicted_frames'], good['predicted_frames'])
        np.testing.assert_array_equal(again['predicted_states'], good['predicted_states'])

    with torch.cuda.device(p0.device):
        st = p0._stream()
        cf, cs, ca, _ = p0._ctx
        d = torch.zeros((2, 1, H, W, 1), dtype=torch.float32, device=p0.device)
        refused(lib.vf_set_context(h, cf.data_ptr(), cs.data_ptr(), ca.data_ptr(), d.data_ptr(), st))
        still_good()
        acts = torch.from_numpy(actions.astype(np.float32)).to(p0.device)
        sc = torch.full((M,), -7.0, dtype=torch.float64, device=p0.device)
        pt = torch.full((M, 1), -7.0, dtype=torch.float64, device=p0.device)
        goal = (ctypes.c_int32 * 2)(3, 4)
        tw = (ctypes.c_float * 1)(1.0)
        fw = ctypes.c_float(1.0)
        for args in ((goal, fw, None, None, None), (None, fw, tw, None, None), (None, fw, None, sc.data_ptr(), None),
                     (None, fw, None, None, pt.data_ptr()), (goal, fw, tw, sc.data_ptr(), pt.data_ptr())):
            refused(lib.vf_rollout(h, acts.data_ptr(), M, *(args + (st,))))
        _lib.check(lib.vf_rollout(h, acts.data_ptr(), M, None, fw, None, None, None, st))       # the frames-only call
        out_d = torch.full((M, T, 1, H, W, 1), -7.0, dtype=torch.float32, device=p0.device)
        out_f = torch.zeros((M, T, 1, H, W, 3), dtype=torch.float32, device=p0.device)
        refused(lib.vf_export(h, 0, M, out_f.data_ptr(), out_d.data_ptr(), None, st))
        _lib.check(lib.vf_export(h, 0, M, out_f.data_ptr(), None, None, st))
        np.testing.assert_array_equal(out_f.cpu().numpy(), good['predicted_frames'])
        seq = torch.arange(2, dtype=torch.int32, device=p0.device)
        lut = torch.zeros((256, 3), dtype=torch.uint8, device=p0.device)
        r_d = torch.full((2, 1, 1, T, H, W, 3), 9, dtype=torch.uint8, device=p0.device)
        r_f = torch.zeros((2, 1, T, H, W, 3), dtype=torch.uint8, device=p0.device)
        refused(lib.vf_render_plans(h, seq.data_ptr(), 2, lut.data_ptr(), r_f.data_ptr(), r_d.data_ptr(), st))
        _lib.check(lib.vf_render_plans(h, seq.data_ptr(), 2, None, r_f.data_ptr(), None, st))    # frames need no colour table
        members = (ctypes.c_void_p * 2)(h.value, h.value)
        refused(lib.vf_ensemble_scores(members, 2, ctypes.c_float(0.1), fw, None, sc.data_ptr(), None, None, st))
        torch.cuda.synchronize(p0.device)
        assert (sc.cpu().numpy() == -7.0).all() and (pt.cpu().numpy() == -7.0).all()        # nothing was written
        assert (out_d.cpu().numpy() == -7.0).all() and (r_d.cpu().numpy() == 9).all()
        np.testing.assert_array_equal(r_f.cpu().numpy(), p0.render_plans(np.arange(2), distributions=False)['frames'])
        # the debug layer entry and the status word work on such a handle as on any other
        status = ctypes.c_int32(5)
        _lib.check(lib.vf_device_status(h, ctypes.byref(status)))
        assert status.value == 0
    still_good()
    # the Python surface
    goal_pix = np.array([[[3, 4]]])
    for call in (lambda: p0.score(ctx0, {'actions': actions}, goal_pix),
                 lambda: p0.fetch_pixel_distributions(0),
                 lambda: p0.render_plans(np.arange(2), frames=True, distributions=True),
                 lambda: p0.render_plans(np.arange(2)),
                 lambda: p0(ctx1, {'actions': actions}),
                 lambda: p0.score_goal_image(ctx1, {'actions': actions}, np.zeros((H, W, 3), np.float32)),
                 lambda: p0.predictor_func()(input_images=ctx0['context_frames'][-2:][None],
                                             input_one_hot_images=ctx1['context_pixel_distributions'][None],
                                             input_state=ctx0['context_states'][-2:][None],
                                             input_actions=np.zeros((M, T + 1, 4)))):
        with pytest.raises(ValueError, match='frames-only'):
            call()
        still_good()
    from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor
    hp = dict(run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W, sequence_length=T + 2, num_ensembles=2)
    with pytest.raises(ValueError, match='frames-only'):
        EnsembleHipPredictor('', dict(hp, designated_pixel_count=0))
    with pytest.raises(ValueError, match='frames-only'):
        EnsembleHipPredictor('', dict(hp, no_pix_distrib=''))
    # register is unaffected
    cur = rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    flow = rs.normal(0, 1, (1, H, W, 2)).astype(np.float32)
    for a, b in zip(p0.register(cur, cur[:, ::-1].copy(), flow, [[[10, 12]]]), p1.register(cur, cur[:, ::-1].copy(), flow, [[[10, 12]]])):
        np.testing.assert_array_equal(a, b)
    # the one-pixel engine still refuses what it refused
    with torch.cuda.device(p1.device):
        rc = p1._libh.vf_set_context(p1._handle, cf.data_ptr(), cs.data_ptr(), ca.data_ptr(), None, p1._stream())
        assert rc == -1 and 'null' in p1._libh.vf_last_error().decode()
    still_good()
    # the bare key of the reference's conf files, and the forcing subclass
    hp = dict(run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W, sequence_length=T + 2)
    for other in (HipVPredEvaluation('', dict(hp, no_pix_distrib='', designated_pixel_count=1)),
                  FramesOnlyHipVPredEvaluation('', dict(hp, designated_pixel_count=1))):
        assert other.frames_only and other.cfg.ndesig == 0
        got = other.restore(w[0])(ctx0, {'actions': actions})
        np.testing.assert_array_equal(got['predicted_frames'], good['predicted_frames'])
        assert other.device_status() == 0


def test_an_abandoned_launch_still_poisons_the_frame_costs():
    H = W = 32
    M = 5
    p0, _, _ = _pair('cdna', H, W, M)
    rs = np.random.RandomState(2)
    ctx0, _ = _contexts(H, W, 4, rs)
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.uniform(0, 1, (H, W, 3)).astype(np.float32)
    good, _ = p0.score_goal_image(ctx0, {'actions': actions}, goal)
    _lib.check(p0._libh.vf_debug_poison_status(p0._handle))
    with pytest.raises(_lib.VfError, match='device status 1'):
        p0.score_goal_image(ctx0, {'actions': actions}, goal)
    assert p0.device_status() == 0
    np.testing.assert_array_equal(p0.score_goal_image(ctx0, {'actions': actions}, goal)[0], good)
    _lib.check(p0._libh.vf_debug_poison_status(p0._handle))
    with pytest.raises(_lib.VfError, match='device status 1'):
        p0(ctx0, {'actions': actions})
    assert p0.device_status() == 0


def test_arch_3_refuses_zero_designated_pixels():
    """The published SAVP generator's heads (vf_savp3.h) have no frames-only form: ``vf_create`` says so."""
    lib = _lib.load_library()
    cfg = _lib.VfConfig(64, 64, 12, 5, 0, 2, 5, 4, 4, 0, 0, 1, 1, 3, 8, 0)
    h = ctypes.c_void_p()
    rc = lib.vf_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = lib.vf_last_error().decode()
    assert rc == -1 and not h.value and 'arch 3' in msg and 'frames-only' in msg, msg
    cfg.ndesig = 5
    assert lib.vf_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and '0..4' in lib.vf_last_error().decode()
    with pytest.raises(ValueError, match='frames-only'):
        HipVPredEvaluation('', dict(arch='savp3', designated_pixel_count=0, adim=12, run_batch_size=4, sequence_length=5))


# ---------------------------------------------------------------------------------------- 5. controllers
class _Worker(object):
    def __init__(self):
        self.messages = []

    def put(self, message):
        self.messages.append(message)


def _with_transformation(base, transformation):
    class Selected(base):
        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(Selected, self).__init__(model_path, dict(hparams, transformation=transformation), n_gpus, first_gpu)
    return Selected


@pytest.mark.parametrize('kind', ['classifier', 'nce', 'goal_image'])
@pytest.mark.parametrize('H,W,transformation', [(32, 32, 'cdna'), (48, 64, 'flow')])
def test_a_planning_call_is_the_same_with_either_predictor_class(kind, H, W, transformation):
    from visual_foresight_amd.policy.cem_controllers import GoalImController
    from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController, NCECostController
    cls = {'classifier': ClassifierController, 'nce': NCECostController, 'goal_image': GoalImController}[kind]
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W}
    pol = {'num_samples': 16, 'iterations': 2, 'repeat': 1, 'rejection_sampling': False, 'nactions': T}
    rs = np.random.RandomState(2)
    frames = rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal = rs.uniform(0, 1, (1, 1, H, W, 3)).astype(np.float32)
    kw = {'classifier': {}, 'nce': {'goal_image': goal}, 'goal_image': {'goal_image': goal[0]}}[kind]
    runs = []
    for base in (FramesOnlyHipVPredEvaluation, HipVPredEvaluation):
        worker = _Worker()
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = cls(dict(ag), dict(pol, predictor_class=_with_transformation(base, transformation)), 0, 1)
            ctrl.reset()
            np.random.seed(0)
            ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1], **kw)
            out = ctrl.act(t=1, i_tr=0, images=frames, state=states, verbose_worker=worker, **kw)
        assert ctrl.predictor.device_status() == 0
        assert ctrl.predictor.cfg.transformation == transformation
        runs.append((ctrl, out, worker))
    (c0, o0, w0), (c1, o1, w1) = runs
    assert c0.predictor.frames_only and c0.predictor.cfg.ndesig == 0 and not c1.predictor.frames_only
    for itr in range(2):
        s0, s1 = o0['plan_stat']['scores_itr%d' % itr], o1['plan_stat']['scores_itr%d' % itr]
        assert s0.shape == (16,) and len(np.unique(s0)) == 16
        np.testing.assert_array_equal(s0, s1)
    np.testing.assert_array_equal(c0._best_indices, c1._best_indices)
    np.testing.assert_array_equal(o0['actions'], o1['actions'])
    np.testing.assert_array_equal(c0.cost_perstep, c1.cost_perstep)
    assert any(m[0] == 'mov' for m in w0.messages)
    assert_same_messages(w0.messages, w1.messages)


# ---------------------------------------------------------------------------------------- 6. memory
def test_the_frames_only_handle_allocates_less_by_at_least_the_distribution_tensors():
    """``hipMemGetInfo`` around ``vf_create`` in a fresh process, 64 x 64, T 13, 200 samples.  The bound is derived: the
    predicted distributions alone are ``max_batch x T x ncam x H x W x 4`` bytes; the context distributions and the block
    sums the frames-only handle also leaves out come on top."""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'helpers', 'frames_only_memory_worker.py'),
                          '64', '64', '13', '200'], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    b0, b1, want = res['bytes']['0'], res['bytes']['1'], res['distrib_bytes']
    print('device bytes: frames-only %d, one designated pixel %d, difference %d (distribution tensors %d)' % (b0, b1, b1 - b0, want))
    assert want == 200 * 13 * 64 * 64 * 4
    assert b0 > 0 and b1 - b0 >= want
