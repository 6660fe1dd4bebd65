"""Learned-cost planning on the host: the frame-scorer table, its oracle, the reference's cost arithmetic (pinned by
``tests/golden/learned_cost.*``, minted by ``tools/make_golden_learned_cost.py`` from the reference's own
``ClassifierController`` / ``NCECostController``), both controllers on their host fallback, and the CPU-checkable parts of
the ``vf_scorer_*`` entry points."""
import contextlib
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import learned_cost_fixtures as fx
from tests.helpers import oracle_frame_scorer as ora
from tests.helpers.fake_frame_predictor import make_fake_frame_predictor_class
from visual_foresight_amd import _lib
from visual_foresight_amd.policy.cem_controllers.cem_base_controller import CEM_HPARAMS
from visual_foresight_amd.policy.cem_controllers.variants import ClassifierController, NCECostController
from visual_foresight_amd.policy.policy import get_policy_args
from visual_foresight_amd.video_prediction import frame_scorer_arch as arch
from visual_foresight_amd.video_prediction.frame_scorer import HostFrameScorer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


@contextlib.contextmanager
def _quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'learned_cost.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'learned_cost.npz'))


# ---------------------------------------------------------------------------------------- the controllers
AG = {'adim': 4, 'sdim': 5, 'image_height': 16, 'image_width': 32}
CLASSES = {'classifier': ClassifierController, 'nce': NCECostController}


def _controller(kind, ncam=1, T=5, **pol):
    fake = make_fake_frame_predictor_class(T, AG['image_height'], AG['image_width'], ncam=ncam)
    pol = dict(dict(repeat=1, rejection_sampling=False, verbose=False, num_samples=30, predictor_class=fake), **pol)
    if T != 5:
        pol['nactions'] = T
    if pol.get('finalweight') == 100:           # (an override equal to the default is refused, as in the reference)
        del pol['finalweight']
    with _quiet():
        ctrl = CLASSES[kind](dict(AG, ncam=ncam), pol, 0, 1)
        ctrl.reset()
    return ctrl


@pytest.mark.parametrize('kind', ['classifier', 'nce'])
def test_defaults_equal_the_reference(golden, kind):
    """Every hyper-parameter the reference defines (classifier_controller.py:66-81, nce_cost_controller.py:65-81 and the CEM
    base / sampler defaults below them) has the reference's default."""
    meta, _ = golden
    vals = _controller(kind)._default_hparams().values()
    want = meta['default_hparams'][kind]
    assert len(want) > 20
    for k, v in want.items():
        assert k in vals, k
        assert vals[k] == v, (k, vals[k], v)
    assert vals['vpred_batch_size'] == 200 and vals['model_path'] == '' and vals['predictor_class'] is None
    for k, v in CEM_HPARAMS:
        assert vals[k] == v or vals[k] is v, k


def test_weight_scores_reproduce_the_reference(golden):
    meta, arrays = golden
    raw = arrays['weight/raw']
    for kind in CLASSES:
        for fw in meta['weight_finalweights']:
            want = arrays['weight/%s/fw%d' % (kind, fw)]
            ctrl = _controller(kind, T=raw.shape[1], finalweight=fw)
            np.testing.assert_allclose(ctrl._weight_scores(raw), want, rtol=1e-12)
            np.testing.assert_allclose(ora.weight_scores(raw, fw), want, rtol=1e-12)
            np.testing.assert_allclose(arch.weight_scores(raw, fw), want, rtol=1e-12)
    np.testing.assert_array_equal(arrays['weight/nce/fw-1'], raw[:, -1])


def test_eval_embedding_cost_reproduces_the_reference(golden):
    _, arrays = golden
    goal, inp, want = arrays['embed/goal'], arrays['embed/input'], arrays['embed/cost']
    ctrl = _controller('nce')
    np.testing.assert_allclose(ctrl._eval_embedding_cost(goal, inp), want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ora.embedding_raw(goal, inp[:, :, None]), want, rtol=1e-12, atol=1e-14)
    ctrl._hp.score_fn = 'cosine'
    with pytest.raises(NotImplementedError):
        ctrl._eval_embedding_cost(goal, inp)
    with pytest.raises(NotImplementedError):
        ctrl.act(t=0, i_tr=0, goal_image=np.zeros((1, 1, 16, 32, 3), np.float32), images=np.zeros((1, 1, 16, 32, 3), np.uint8),
                 state=np.zeros((1, 5)))


def _case_head_outputs(case):
    """What the reference's fake scoring functions saw and returned in a golden case, rebuilt from the seed: head
    outputs ``[M, T, ncam, D]`` as float32 (logits resp. embeddings) and ``goal_enc [ncam, D]``."""
    c = case
    inp = fx.case_inputs(c['seed'], c['ncam'], c['H'], c['W'], c['M'], c['T'], c['adim'], c['sdim'], c['n_context'])
    actions = inp['actions']
    if c['controller'] == 'classifier':         # the reference prepends the context actions and cuts to seqlen (:84-86)
        prev = np.tile(np.stack(inp['chosen_actions'][-c['n_context']:])[None], [c['M'], 1, 1])
        actions = np.concatenate((prev, actions), axis=1)[:, :c['T'] + c['n_context']]
    frames = fx.fake_frames(c['seed'], actions, c['T'], c['ncam'], c['H'], c['W'])          # in [0, 1]
    heads, goal_enc = [], None
    for cam in range(c['ncam']):
        flat = frames[:, :, cam].reshape((-1, c['H'], c['W'], 3))
        if c['controller'] == 'classifier':
            heads.append(fx.classifier_logits(c['seed'], (flat * 255.) / 255))
        else:
            heads.append(fx.embed_frames(c['seed'], flat * 255.))
    head_out = np.stack(heads, axis=1).reshape(c['M'], c['T'], c['ncam'], -1)
    if c['controller'] == 'nce':
        goal, start = inp['goal_image'][-1] * 255, inp['images'][-1].astype(np.float32)
        goal_enc = np.concatenate([fx.embed_goal(c['seed'], goal[cam][None], start[cam][None]) for cam in range(c['ncam'])])
    return head_out, goal_enc


def test_evaluate_rollouts_arithmetic_reproduces_the_reference(golden):
    """The reference's ``evaluate_rollouts`` driven whole (fake predictor, fake scorer): ``-log(p + 1e-5)`` resp. the inner
    product, the SUM over views, the ``* 255`` scaling and ``_weight_scores`` - against the package's host arithmetic, the
    controllers' methods and the oracle helper, to float64 round-off."""
    meta, arrays = golden
    assert int(meta['numpy'].split('.')[0]) >= 1
    for case in meta['cases']:
        assert case['dtype'] == 'float64'
        want = arrays[case['name'] + '/scores']
        head_out, goal_enc = _case_head_outputs(case)
        head = 'classifier' if case['controller'] == 'classifier' else 'embedding'
        got, cps = arch.learned_cost(head, head_out, goal_enc, case['finalweight'])
        np.testing.assert_allclose(got, want, rtol=1e-12, err_msg=case['name'])
        got_o, cps_o = ora.learned_cost(head, head_out, goal_enc, case['finalweight'])
        np.testing.assert_allclose(got_o, want, rtol=1e-12, err_msg=case['name'])
        np.testing.assert_allclose(cps, cps_o, rtol=1e-12)
        ctrl = _controller(case['controller'], ncam=case['ncam'], T=case['T'], finalweight=case['finalweight'])
        raw = ctrl._raw_scores(head_out, goal_enc)
        np.testing.assert_allclose(ctrl._weight_scores(raw), want, rtol=1e-12, err_msg=case['name'])
        assert len(np.unique(want)) == len(want)


def test_draw_mean_of_the_cost_helpers():
    rs = np.random.RandomState(1)
    head_out = rs.normal(0, 1, (6, 4, 2, 2)).astype(np.float32)
    s, cps = arch.learned_cost('classifier', head_out, None, 3., n_draws=3)
    s1, cps1 = arch.learned_cost('classifier', head_out, None, 3., n_draws=1)
    np.testing.assert_allclose(s, s1.reshape(2, 3).mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(cps, cps1.reshape(2, 3, 4).mean(axis=1), rtol=1e-13)
    so, cpo = ora.learned_cost('classifier', head_out, None, 3., n_draws=3)
    np.testing.assert_allclose(s, so, rtol=1e-13)
    np.testing.assert_allclose(cps, cpo, rtol=1e-13)


@pytest.mark.parametrize('kind,ncam', [('classifier', 1), ('classifier', 2), ('nce', 1), ('nce', 2)])
def test_three_iteration_act_on_the_host_fallback(kind, ncam):
    H, W, T = AG['image_height'], AG['image_width'], 5
    ctrl = _controller(kind, ncam=ncam, finalweight=4)
    assert isinstance(ctrl.scorer, HostFrameScorer) and ctrl._hp.start_planning == 1
    rs = np.random.RandomState(9)
    images = rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    kw = {'goal_image': rs.uniform(0, 1, (2, ncam, H, W, 3)).astype(np.float32)} if kind == 'nce' else {}
    np.random.seed(0)
    with _quiet():
        ctrl.act(t=0, i_tr=0, images=images[:1], state=states[:1], **kw)
        out = ctrl.act(t=1, i_tr=0, images=images, state=states, **kw)
    assert out['actions'].shape == (4,)
    assert sorted(out['plan_stat']) == ['scores_itr0', 'scores_itr1', 'scores_itr2']
    pred = ctrl.predictor
    assert len(pred.actions_seen) == 3 and pred.contexts[0]['context_pixel_distributions'] == (2, ncam, H, W, 1)
    # the scores are the oracle's on the frames the predictor returned
    other = make_fake_frame_predictor_class(T, H, W, ncam=ncam)('', {})
    head = ctrl.scorer.cfg.head
    goal_enc = None
    if kind == 'nce':
        pair = np.concatenate([kw['goal_image'][-1], images[-1].astype(np.float32) / np.float32(255.)], axis=-1)
        goal_enc = ora.forward_views(ctrl.scorer.weights['goal'], pair[None], 255., torch.float32)[0]
    for itr, actions in enumerate(pred.actions_seen):
        frames = other({'context_frames': images}, {'actions': actions})['predicted_frames']
        enc = ora.forward_views(ctrl.scorer.weights['frames'], frames.reshape((-1,) + frames.shape[2:]),
                                ctrl.scorer.cfg.input_scale, torch.float32).reshape(frames.shape[:3] + (-1,))
        want, want_cps = ora.learned_cost(head, enc, goal_enc, 4)
        np.testing.assert_allclose(out['plan_stat']['scores_itr%d' % itr], want, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ctrl.cost_perstep, want_cps, rtol=1e-4, atol=1e-6)
    assert ctrl._best_indices.shape == (10,)


def test_policy_args_bind_the_goal_image_by_name():
    ctrl = _controller('nce')
    images, state = np.zeros((1, 1, 16, 32, 3), np.uint8), np.zeros((1, 5))
    goal = np.ones((1, 1, 16, 32, 3), np.float32)
    kw = get_policy_args(ctrl, {'images': images, 'state': state}, 0, 0, {'goal_image': goal})
    assert kw['goal_image'] is goal and kw['images'] is images and kw['verbose_worker'] is None
    kw = get_policy_args(_controller('classifier'), {'images': images, 'state': state}, 0, 0, {'goal_image': goal})
    assert 'goal_image' not in kw and kw['images'] is images


def test_import_paths_mirror_the_reference():
    import importlib
    a = importlib.import_module('visual_foresight_amd.policy.cem_controllers.variants.classifier_controller')
    b = importlib.import_module('visual_foresight_amd.policy.cem_controllers.variants.nce_cost_controller')
    assert a.ClassifierController is ClassifierController and b.NCECostController is NCECostController


# ---------------------------------------------------------------------------------------- the table
def test_macs_and_weight_count():
    cfg = arch.FrameScorerConfig()
    macs = cfg.macs_per_frame()
    assert sum(macs.values()) == pytest.approx(12.69e6, rel=1e-3)
    assert [macs['c%d' % i] for i in (1, 2, 3, 4)] == [884736, 4718592, 4718592, 2359296]
    n = sum(int(np.prod(s)) for s in cfg.tensor_shapes().values())
    assert n == 241090 and arch.FrameScorerWeights.random(cfg).n_floats() == n
    emb = arch.FrameScorerConfig(head='embedding', embed_dim=64)
    assert emb.input_scale == 255. and cfg.input_scale == 1.
    assert emb.tensor_shapes('goal')['c1/w'] == (3, 3, 6, 32) and emb.tensor_shapes()['fc/w'] == (128, 64)
    with pytest.raises(ValueError):
        cfg.tensor_shapes('goal')               # the classifier has no goal tower
    with pytest.raises(ValueError):
        arch.FrameScorerConfig(height=40)


def test_weights_roundtrip_and_refusals(tmp_path):
    cfg = arch.FrameScorerConfig(height=32, width=48, head='embedding', embed_dim=16)
    ws = arch.random_scorer_weights(cfg, ncam=2, seed=3, bias_scale=0.2)
    assert ws['frames'][0].tensors['c1/b'].std() > 0
    arch.save_scorer_weights(ws, str(tmp_path))
    back = arch.load_scorer_weights(str(tmp_path), cfg, ncam=2)
    for tw in ('frames', 'goal'):
        for a, b in zip(ws[tw], back[tw]):
            assert list(a.tensors) == list(b.tensors)
            for k in a.tensors:
                np.testing.assert_array_equal(a.tensors[k], b.tensors[k])
    again = arch.random_scorer_weights(cfg, ncam=2, seed=3, bias_scale=0.2)
    np.testing.assert_array_equal(again['goal'][1].blob(), ws['goal'][1].blob())
    view0 = os.path.join(str(tmp_path), 'frames', 'view0')
    with pytest.raises(ValueError):             # another head
        arch.FrameScorerWeights.load(view0, arch.FrameScorerConfig(height=32, width=48))
    with pytest.raises(ValueError):             # another size
        arch.FrameScorerWeights.load(view0, arch.FrameScorerConfig(height=64, width=48, head='embedding', embed_dim=16))
    with pytest.raises(ValueError):             # another embedding width
        arch.FrameScorerWeights.load(view0, arch.FrameScorerConfig(height=32, width=48, head='embedding', embed_dim=8))
    with pytest.raises(ValueError):             # the other tower
        arch.FrameScorerWeights.load(view0, cfg, tower='goal')
    with pytest.raises(ValueError):             # a scorer refuses weights of the other head
        HostFrameScorer(ws, {'image_height': 32, 'image_width': 48, 'ncam': 2, 'head': 'classifier'}).restore()


@pytest.mark.parametrize('H,W,head,D', [(64, 64, 0, 2), (48, 64, 1, 64), (128, 128, 1, 16)])
def test_library_weight_count_agrees_with_the_table(H, W, head, D):
    _lib.build_library()
    lib = _lib.load_library()
    cfg = arch.FrameScorerConfig(height=H, width=W, head=arch.HEADS[head], embed_dim=D)
    c = _lib.VfScorerConfig(H, W, 1, head, D, 10, 0, 1.0)
    for i, tw in enumerate(cfg.towers):
        n = sum(int(np.prod(s)) for s in cfg.tensor_shapes(tw).values())
        assert lib.vf_scorer_weight_count(ctypes.byref(c), i) == n
    assert lib.vf_scorer_weight_count(ctypes.byref(c), head + 1) == 0 and b'tower' in lib.vf_last_error()
    bad = _lib.VfScorerConfig(40, 64, 1, 0, 2, 10, 0, 1.0)
    assert lib.vf_scorer_weight_count(ctypes.byref(bad), 0) == 0 and b'multiples of 16' in lib.vf_last_error()


def test_header_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'vf_hip.h')).read()
    declared = set(re.findall(r'\b(vf_[a-z_]+)\s*\(', header))
    assert declared == set(_lib.EXPORTS)
    for name in ('vf_scorer_weight_count', 'vf_scorer_create', 'vf_scorer_destroy', 'vf_scorer_load_weights',
                 'vf_scorer_embed', 'vf_scorer_scores'):
        assert name in declared
    assert re.search(r'#define VF_ABI_VERSION 7\b', header)
    _lib.build_library()
    lib = _lib.load_library()
    # refusals that need no device: nothing is dereferenced, no HIP call is made
    out = (ctypes.c_double * 4)()
    assert lib.vf_scorer_scores(None, None, None, 100., ctypes.cast(out, ctypes.c_void_p), None, None, None) == -1
    assert b'null' in lib.vf_last_error()
    assert lib.vf_scorer_embed(None, 0, None, 1, None, None) == -1
    assert lib.vf_scorer_create(None, None) == -1


# ---------------------------------------------------------------------------------------- the oracle
def test_oracle_blocks_against_naive_loops():
    rs = np.random.RandomState(2)
    x = rs.uniform(-1, 1, (2, 6, 8, 3))
    w, b = rs.uniform(-1, 1, (3, 3, 3, 5)), rs.uniform(-1, 1, 5)
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-5)):
        got = ora.conv_block(torch.from_numpy(x).to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)).numpy()
        np.testing.assert_allclose(got, ora.naive_conv_block(x, w, b), rtol=tol, atol=tol)
    assert (ora.naive_conv_block(x, w, b) == 0).any()           # the ReLU does cut
    y = rs.uniform(0, 1, (2, 3, 4, 5))
    np.testing.assert_allclose(ora.pool_block(torch.from_numpy(y)).numpy(), ora.naive_pool_block(y), rtol=1e-13)
    fw, fb = rs.uniform(-1, 1, (5, 3)), rs.uniform(-1, 1, 3)
    got = ora.fc_block(torch.from_numpy(y[:, 0, 0]), torch.from_numpy(fw), torch.from_numpy(fb)).numpy()
    want = np.array([[sum(y[i, 0, 0, k] * fw[k, d] for k in range(5)) + fb[d] for d in range(3)] for i in range(2)])
    np.testing.assert_allclose(got, want, rtol=1e-13)


def test_oracle_precisions_host_scorer_and_device_order_agree():
    """float64 vs float32 oracle vs the package's host scorer vs the float32 chain in the device's K order: all within
    float32 round-off of each other; the device-order restatement differs from PyTorch's float32 in order only."""
    cfg = arch.FrameScorerConfig(height=32, width=32, head='embedding', embed_dim=8)
    ws = arch.random_scorer_weights(cfg, ncam=1, seed=4, bias_scale=0.1)
    imgs = np.random.RandomState(3).uniform(0, 1, (3, 1, 32, 32, 3)).astype(np.float32)
    f64 = ora.forward_views(ws['frames'], imgs, cfg.input_scale, torch.float64)
    f32 = ora.forward_views(ws['frames'], imgs, cfg.input_scale, torch.float32)
    dev = ora.forward_device_order(ws['frames'][0], imgs[:, 0], cfg.input_scale)[:, None]
    host = HostFrameScorer(ws, {'image_height': 32, 'image_width': 32, 'head': 'embedding', 'embed_dim': 8}).restore().embed(imgs)
    scale = np.abs(f64).max()
    assert scale > 1.0
    for other in (f32, dev, host):
        assert np.abs(other - f64).max() / scale < 2e-5
    np.testing.assert_array_equal(host, f32)
    assert ora.device_k_order(16, False) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]
