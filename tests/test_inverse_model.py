"""CPU checks of the inverse-model policy: the table of ``inverse_model_arch.py`` and its files, the torch restatement
against naive loops, ``HostActionInference`` against the restatement, ``InvModelBaseController`` against traces of the
reference's own controller (``tests/golden/inverse_model.*``, minted by ``tools/make_golden.py`` with the fake predictor of
``tests/helpers/fake_action_inference.py`` on both sides), and the C ABI's new names."""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests.helpers import oracle_inverse_model as ora                                                   # noqa: E402
from tests.helpers.fake_action_inference import make_fake_action_inference                              # noqa: E402
from visual_foresight_amd import _lib                                                                   # noqa: E402
from visual_foresight_amd.policy.inverse_models import InvModelBaseController, convert_to_float         # noqa: E402
from visual_foresight_amd.video_prediction.inverse_model import HostActionInference                     # noqa: E402
from visual_foresight_amd.video_prediction.inverse_model_arch import InverseModelConfig, InverseModelWeights  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def problem(cfg, seed, n=1):
    rs = np.random.RandomState(seed)
    img = (cfg.height, cfg.width, 3)
    return (rs.uniform(0, 1, (n,) + img).astype(np.float32), rs.uniform(0, 1, (n,) + img).astype(np.float32),
            rs.uniform(-1, 1, (n, cfg.n_context, cfg.adim)).astype(np.float32),
            rs.uniform(0, 1, (n, cfg.n_context) + img).astype(np.float32))


# ------------------------------------------------------------------------------------------------------ table and files
def test_tensor_table_and_weight_count():
    cfg = InverseModelConfig(height=48, width=64, adim=5, n_context=3, n_actions=7)
    shapes = cfg.tensor_shapes()
    names = ['%s/c%d/%s' % (tw, l, k) for tw in ('pair', 'ctx') for l in (1, 2, 3, 4) for k in ('w', 'b')]
    assert list(shapes) == names + ['lstm/wx', 'lstm/wa', 'lstm/wh', 'lstm/b', 'out/w', 'out/b']
    assert shapes['pair/c1/w'] == (3, 3, 6, 32) and shapes['ctx/c1/w'] == (3, 3, 3, 32)
    assert shapes['pair/c4/w'] == shapes['ctx/c4/w'] == (3, 3, 128, 128)
    assert shapes['lstm/wx'] == shapes['lstm/wh'] == (128, 512) and shapes['lstm/wa'] == (5, 512) and shapes['lstm/b'] == (512,)
    assert shapes['out/w'] == (128, 5) and shapes['out/b'] == (5,)
    tower = lambda cin: 9 * (cin * 32 + 32 * 64 + 64 * 128 + 128 * 128) + 32 + 64 + 128 + 128
    assert cfg.n_floats() == tower(6) + tower(3) + (128 + 5 + 128 + 1) * 512 + 128 * 5 + 5
    w = InverseModelWeights.random(cfg, seed=3)
    assert w.n_floats() == cfg.n_floats() == w.blob().size and w.blob().dtype == np.float32
    again = InverseModelWeights.random(cfg, seed=3)
    for k in w.tensors:
        np.testing.assert_array_equal(w.tensors[k], again.tensors[k])
    for bad in (dict(height=40), dict(width=144), dict(adim=0), dict(adim=9), dict(n_context=0), dict(n_context=5),
                dict(n_actions=0), dict(n_actions=33), dict(input_scale=0.0)):
        with pytest.raises(ValueError):
            InverseModelConfig(**bad)


def test_weights_file_roundtrip_and_refusals(tmp_path):
    cfg = InverseModelConfig(height=32, width=48, adim=3, n_context=2, n_actions=5, input_scale=2.0)
    w = InverseModelWeights.random(cfg, seed=5)
    w.save(str(tmp_path))
    manifest = json.load(open(str(tmp_path / 'manifest.json')))
    assert manifest['format'] == 'vf-inverse-model-v1' and manifest['n_floats'] == cfg.n_floats()
    r = InverseModelWeights.load(str(tmp_path))
    assert r.cfg.as_dict() == cfg.as_dict() and list(r.tensors) == list(w.tensors)
    for k in w.tensors:
        np.testing.assert_array_equal(w.tensors[k], r.tensors[k])
    InverseModelWeights.load(str(tmp_path), cfg)
    for other in (dict(height=48), dict(width=32), dict(adim=4), dict(n_context=1), dict(n_actions=6)):
        with pytest.raises(ValueError, match='does not match'):
            InverseModelWeights.load(str(tmp_path), InverseModelConfig(**dict(cfg.as_dict(), **other)))
    with open(str(tmp_path / 'weights.bin'), 'ab') as f:
        f.write(b'\0\0\0\0')
    with pytest.raises(ValueError, match='floats'):
        InverseModelWeights.load(str(tmp_path))
    manifest['format'] = 'vf-registration-net-v1'
    json.dump(manifest, open(str(tmp_path / 'manifest.json'), 'w'))
    with pytest.raises(ValueError, match='format'):
        InverseModelWeights.load(str(tmp_path))


# ------------------------------------------------------------------------------------------- restatement and host twin
SMALL = dict(height=16, width=16, adim=2, n_context=1, n_actions=2)


def test_restatement_blocks_against_naive_loops():
    cfg = InverseModelConfig(**SMALL)
    w = InverseModelWeights.random(cfg, seed=1)
    rs = np.random.RandomState(2)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    x = rs.uniform(0, 1, (2, 16, 16, 6))
    got = ora.conv_block(t64(x), t64(w.tensors['pair/c1/w']), t64(w.tensors['pair/c1/b'])).numpy()
    np.testing.assert_allclose(got, ora.naive_conv_block(x, w.tensors['pair/c1/w'], w.tensors['pair/c1/b']), rtol=0, atol=1e-13)
    assert got.shape == (2, 8, 8, 32) and (got > 0).any() and (got == 0).any()
    feat = rs.uniform(0, 1, (2, 3, 5, 128))
    np.testing.assert_allclose(feat.reshape(2, -1, 128).mean(axis=1), ora.naive_pool_block(feat), rtol=0, atol=1e-14)
    lstm = {k: t64(w.tensors[k]) for k in ('lstm/wx', 'lstm/wa', 'lstm/wh', 'lstm/b')}
    xv, av, hv, cv = rs.uniform(0, 1, 128), rs.uniform(-1, 1, 2), rs.uniform(-1, 1, 128), rs.uniform(-1, 1, 128)
    for order in (0, 1):
        h2, c2 = ora.cell_block(t64(xv)[None], t64(av)[None], t64(hv)[None], t64(cv)[None], lstm, order)
        nh, nc = ora.naive_cell_block(xv, av, hv, cv, *(w.tensors[k] for k in ('lstm/wx', 'lstm/wa', 'lstm/wh', 'lstm/b')))
        np.testing.assert_allclose(h2.numpy()[0], nh, rtol=0, atol=1e-13)
        np.testing.assert_allclose(c2.numpy()[0], nc, rtol=0, atol=1e-13)
    # the whole schedule: warm-up on the context, the last context action fed to the first decode step
    start, goal, ca, cf = problem(cfg, 3)
    actions, hidden = ora.forward(w, start, goal, ca, cf, torch.float64)
    n_act, n_hid = ora.naive_forward(w, start[0], goal[0], ca[0], cf[0])
    assert actions.shape == (1, 2, 2) and hidden.shape == (1, 3, 2, 128)
    np.testing.assert_allclose(actions[0], n_act, rtol=0, atol=1e-12)
    np.testing.assert_allclose(hidden[0], n_hid, rtol=0, atol=1e-12)


@pytest.mark.parametrize('H,W,adim,nc,na,n', [(16, 16, 2, 1, 2, 1), (32, 48, 5, 3, 7, 2)])
def test_host_twin_against_the_float32_restatement(H, W, adim, nc, na, n):
    cfg = InverseModelConfig(height=H, width=W, adim=adim, n_context=nc, n_actions=na, input_scale=1.5)
    w = InverseModelWeights.random(cfg, seed=4)
    host = HostActionInference(w, {}).restore()
    start, goal, ca, cf = problem(cfg, 5, n)
    got, hid = host.infer(start, goal, ca, cf, want_hidden=True)
    want, want_hid = ora.forward(w, start, goal, ca, cf, torch.float32)
    assert got.shape == (n, na, adim) and got.dtype == np.float32
    # the same float32 table through the same library: equal up to the library's choice of summation order
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    np.testing.assert_allclose(hid, want_hid, rtol=0, atol=2e-5)
    f64, _ = ora.forward(w, start, goal, ca, cf, torch.float64)
    assert np.abs(got - f64).max() < 1e-4 * max(1.0, np.abs(f64).max())
    # the reference's call: one problem without the batch axis on the images
    one = host(start[0], goal[0], ca[:1], cf[:1])
    np.testing.assert_array_equal(one, host.infer(start[:1], goal[:1], ca[:1], cf[:1]))
    assert one.shape == (1, na, adim)
    # float64 inputs (what the controller passes) are taken as their float32 values
    np.testing.assert_array_equal(host(start[0].astype(np.float64), goal[0].astype(np.float64), ca[:1].astype(np.float64),
                                       cf[:1].astype(np.float64)), one)
    with pytest.raises(ValueError, match='%dx%d' % (H, W)):
        host(start[0, :8], goal[0, :8], ca[:1], cf[:1, :, :8])
    with pytest.raises(ValueError, match='restore'):
        HostActionInference(w, {})(start[0], goal[0], ca[:1], cf[:1])


def test_random_weights_give_actions_that_vary_and_follow_the_goal():
    """What the GPU tests rely on: with the seeded random weights the gates are not saturated, the actions change over the
    decode steps and react to the goal image."""
    cfg = InverseModelConfig(height=32, width=32, adim=4, n_context=2, n_actions=8)
    w = InverseModelWeights.random(cfg, seed=0)
    start, goal, ca, cf = problem(cfg, 1)
    actions, hidden = ora.forward(w, start, goal, ca, cf, torch.float32)
    other, _ = ora.forward(w, start, problem(cfg, 2)[1], ca, cf, torch.float32)
    assert np.abs(hidden[:, :, 0]).max() < 0.999                       # |h| stays away from 1
    assert np.ptp(actions[0], axis=0).max() > 1e-2
    assert np.abs(actions - other).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------- controller
def golden():
    with open(os.path.join(GOLDEN, 'inverse_model.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'inverse_model.npz'))


def episodes():
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    try:
        import make_golden
    finally:
        sys.path.pop(0)
    return make_golden


@pytest.mark.parametrize('name', ['replan2', 'replan2_short', 'replan1', 'replan1_short'])
def test_controller_against_the_reference_trace(name):
    """Same action sequences, same recorded predictor arguments (shape, dtype, checksum of every call), the same assertion
    with its text when a plan runs out, the same behaviour before and after ``reset()``."""
    mg = episodes()
    meta, arrays = golden()
    want = meta['episodes'][name]
    (_, seed, overrides, n_plan, steps, steps_again), = [e for e in mg.INVERSE_MODEL_EPISODES if e[0] == name]
    assert (seed, overrides, steps, steps_again) == (want['seed'], want['overrides'], want['steps'], want['steps_again'])
    fake = make_fake_action_inference(n_plan, 4)
    with contextlib.redirect_stdout(io.StringIO()):
        got_arrays, got = mg.run_inverse_model_episode(InvModelBaseController, fake, seed, dict(overrides, predictor_class=fake),
                                                       steps, steps_again)
    assert got['constructed'] == want['constructed']
    assert got['act_before_reset'] == want['act_before_reset'] == 'AttributeError: plan_stat'
    for ep in ('ep0', 'ep1'):
        assert got[ep] == want[ep], ep
    assert len(got['calls']) == len(want['calls'])
    for i, (g, wnt) in enumerate(zip(got['calls'], want['calls'])):
        for arg_g, arg_w in zip(g, wnt):
            assert arg_g['shape'] == arg_w['shape'] and arg_g['dtype'] == arg_w['dtype'], (i, arg_g, arg_w)
            assert arg_g['checksum'] == arg_w['checksum'], (i, arg_g, arg_w)
    keys = [k for k in arrays.files if k.startswith(name + '/')]
    assert sorted(k[len(name) + 1:] for k in keys) == sorted(got_arrays)
    for k in keys:
        np.testing.assert_array_equal(got_arrays[k[len(name) + 1:]], arrays[k], err_msg=k)
    if name.endswith('_short'):
        assert want['ep0']['error']['text'].startswith('Tried to take action')
        assert 'Maybe re-planning is not occurring often enough?' in want['ep0']['error']['text']


def test_controller_defaults_and_predictor_hparams():
    fake = make_fake_action_inference(15, 4)
    ag = {'adim': 4, 'sdim': 5, 'image_height': 48, 'image_width': 64}
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = InvModelBaseController(ag, {'predictor_class': fake, 'num_context': 3, 'T': 9}, 2, 4)
    hp = ctrl._hp.values()
    assert (hp['load_T'], hp['replan_every'], hp['model_params_path'], hp['model_restore_path']) == (7, 2, '', '')
    assert hp['context_action_weight'] == [1, 1, 1, 1] and hp['initial_action_low'] == [-0.025, -0.025, -0.025, 0]
    assert hp['initial_action_high'] == [0.025, 0.025, 0.025, 0] and hp['logging_dir'] == ''
    pred = ctrl.predictor
    assert pred.hparams == {'adim': 4, 'n_context': 3, 'n_actions': 9, 'image_height': 48, 'image_width': 64}
    assert (pred.n_gpus, pred.first_gpu, pred.restored) == (4, 2, 1)
    out = convert_to_float(np.array([[0, 255, 51]], np.uint8))
    assert out.dtype == np.float64 and out.tolist() == [[0.0, 1.0, 0.2]]
    with pytest.raises(AssertionError, match='uint8'):
        convert_to_float(np.zeros(3, np.float32))
    with pytest.raises(ValueError, match='identical to default'):
        InvModelBaseController(ag, {'predictor_class': fake, 'replan_every': 2}, 0, 1)


def test_controller_with_the_host_network(tmp_path):
    """The CPU path end to end: a model directory named by ``model_params_path`` supplies the config."""
    cfg = InverseModelConfig(height=16, width=16, adim=4, n_context=2, n_actions=3)
    InverseModelWeights.random(cfg, seed=6).save(str(tmp_path))
    ag = {'adim': 4, 'sdim': 5, 'image_height': 16, 'image_width': 16}
    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (5, 1, 16, 16, 3)).astype(np.uint8)
    goal = rs.uniform(0, 1, (1, 1, 16, 16, 3))
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = InvModelBaseController(ag, {'predictor_class': HostActionInference, 'model_params_path': str(tmp_path)}, 0, 1)
        ctrl.reset()
        np.random.seed(1)
        outs = [ctrl.act(t=t, i_tr=0, images=frames[:t + 1], goal_image=goal)['actions'] for t in range(5)]
    assert ctrl.predictor.cfg.as_dict() == cfg.as_dict()
    want = ctrl.predictor(frames[2, 0] / 255., goal[-1, 0], np.array(outs[:2])[None], (frames[:2, 0] / 255.)[None])
    np.testing.assert_array_equal(outs[2], want[0, 0])
    np.testing.assert_array_equal(outs[3], want[0, 1])
    assert outs[4].dtype == np.float32 and not np.array_equal(outs[4], want[0, 2])      # replanned at t = 4


# ------------------------------------------------------------------------------------------------------------------ ABI
NEW_EXPORTS = ('vf_invmodel_weight_count', 'vf_invmodel_create', 'vf_invmodel_destroy', 'vf_invmodel_load_weights',
               'vf_invmodel_infer')


def test_header_declarations_equal_the_exports():
    header = open(os.path.join(REPO, 'include', 'vf_hip.h')).read()
    declared = set(re.findall(r'\b(vf_[a-z_]+)\s*\(', header))
    assert declared == set(_lib.EXPORTS)
    assert set(NEW_EXPORTS) <= declared
    assert re.search(r'#define\s+VF_ABI_VERSION\s+7\b', header) and _lib.ABI_VERSION == 7
    block = header[header.index('typedef struct vf_invmodel_config'):header.index('} vf_invmodel_config;')]
    fields = re.findall(r'\b(height|width|adim|n_context|n_actions|max_batch|device|input_scale)\b', block)
    assert fields == [n for n, _ in _lib.VfInvModelConfig._fields_]


def test_library_table_and_refusals_without_a_gpu():
    import ctypes
    _lib.build_library()
    lib = _lib.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    for adim, nc, na in ((4, 2, 15), (1, 4, 32), (8, 1, 1)):
        cfg = InverseModelConfig(height=64, width=64, adim=adim, n_context=nc, n_actions=na)
        c = _lib.VfInvModelConfig(64, 64, adim, nc, na, 2, 0, 1.0)
        assert lib.vf_invmodel_weight_count(ctypes.byref(c)) == cfg.n_floats()
    for bad, msg in ((_lib.VfInvModelConfig(40, 64, 4, 2, 15, 1, 0, 1.0), b'multiples of 16'),
                     (_lib.VfInvModelConfig(64, 144, 4, 2, 15, 1, 0, 1.0), b'at most 128'),
                     (_lib.VfInvModelConfig(64, 64, 9, 2, 15, 1, 0, 1.0), b'adim'),
                     (_lib.VfInvModelConfig(64, 64, 4, 5, 15, 1, 0, 1.0), b'n_context'),
                     (_lib.VfInvModelConfig(64, 64, 4, 2, 33, 1, 0, 1.0), b'n_actions'),
                     (_lib.VfInvModelConfig(64, 64, 4, 2, 15, 0, 0, 1.0), b'max_batch'),
                     (_lib.VfInvModelConfig(64, 64, 4, 2, 15, 1, 0, 0.0), b'input_scale')):
        assert lib.vf_invmodel_weight_count(ctypes.byref(bad)) == 0 and msg in lib.vf_last_error()
        handle = ctypes.c_void_p()
        assert lib.vf_invmodel_create(ctypes.byref(bad), ctypes.byref(handle)) != 0 and not handle.value
    assert lib.vf_invmodel_infer(None, None, None, None, None, 1, None, None, None) != 0 and b'null' in lib.vf_last_error()
    assert lib.vf_invmodel_destroy(None) == 0


def test_device_predictor_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from visual_foresight_amd.video_prediction.inverse_model import HipActionInference
    with pytest.raises(_lib.VfError):
        HipActionInference('', {})
