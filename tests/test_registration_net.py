"""The registration network on the CPU: architecture table, weight files, the gdnconf mapping, the PyTorch restatement
against naive loops, ``HostRegistrationNet`` against the restatement, the vectorised warp against the loop oracle, the
library's bookkeeping, and a planning call of ``RegisterGtruthController`` with the host net as its warper."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import registration as oracle_reg                                              # noqa: E402
from tests.helpers import oracle_registration_net as ora                                   # noqa: E402
from tests.helpers.fake_predictor import make_fake_predictor_class                         # noqa: E402
from visual_foresight_amd import _lib                                                      # noqa: E402
from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController           # noqa: E402
from visual_foresight_amd.policy.cem_controllers.registration import bilinear_warp         # noqa: E402
from visual_foresight_amd.video_prediction import registration_net_arch as arch            # noqa: E402
from visual_foresight_amd.video_prediction.registration_net import HostRegistrationNet     # noqa: E402


def test_arch_table_and_macs():
    cfg = arch.RegistrationNetConfig(64, 64, 4)
    shapes = cfg.tensor_shapes()
    assert list(shapes) == ['d1/w', 'd1/b', 'd2/w', 'd2/b', 'd3/w', 'd3/b', 'u1/w', 'u1/b', 'u2/w', 'u2/b', 'u3/w', 'u3/b',
                            'flow/w', 'flow/b']
    assert shapes['d1/w'] == (3, 3, 6, 128) and shapes['d3/w'] == (3, 3, 256, 512) and shapes['u1/w'] == (3, 3, 512, 256)
    assert shapes['u3/w'] == (3, 3, 128, 64) and shapes['flow/w'] == (5, 5, 64, 2) and shapes['flow/b'] == (2,)
    macs = cfg.macs_per_pair()
    assert macs['u1'] == 64 * 9 * 512 * 256 and macs['flow'] == 64 * 64 * 25 * 64 * 2
    assert sum(macs.values()) == pytest.approx(0.871e9, rel=2e-3)
    assert sum(arch.RegistrationNetConfig(96, 128, 4).macs_per_pair().values()) == pytest.approx(2.61e9, rel=3e-3)
    assert arch.RegistrationNetConfig(48, 64, 1).tensor_shapes()['u3/w'] == (3, 3, 32, 16)
    for bad in ((60, 64, 4), (8, 64, 1), (64, 64, 3), (136, 128, 4), (64, 256, 1)):
        with pytest.raises(ValueError):
            arch.RegistrationNetConfig(*bad)
    with pytest.raises(ValueError, match='up to 128x128'):
        arch.RegistrationNetConfig(64, 136, 1)


def test_weights_roundtrip_and_refusals(tmp_path):
    cfg = arch.RegistrationNetConfig(32, 48, 2)
    views = arch.random_registration_weights(cfg, ncam=2, seed=5, bias_scale=0.1)
    again = arch.random_registration_weights(cfg, ncam=2, seed=5, bias_scale=0.1)
    for a, b in zip(views, again):
        for k in a.tensors:
            np.testing.assert_array_equal(a.tensors[k], b.tensors[k])
    assert not np.array_equal(views[0].tensors['d2/w'], views[1].tensors['d2/w'])       # one network per view
    assert views[0].blob().size == views[0].n_floats() == cfg.n_floats()
    arch.save_registration_weights(views, str(tmp_path))
    assert (tmp_path / 'view1' / 'manifest.json').exists()
    back = arch.load_registration_weights(str(tmp_path), cfg, ncam=2)
    for a, b in zip(views, back):
        assert list(a.tensors) == list(b.tensors)
        for k in a.tensors:
            np.testing.assert_array_equal(a.tensors[k], b.tensors[k])
    with pytest.raises(ValueError, match='ch_mult'):
        arch.RegistrationNetWeights.load(str(tmp_path / 'view0'), arch.RegistrationNetConfig(32, 48, 4))
    with pytest.raises(ValueError, match='height'):
        arch.RegistrationNetWeights.load(str(tmp_path / 'view0'), arch.RegistrationNetConfig(64, 48, 2))
    with open(str(tmp_path / 'view0' / 'weights.bin'), 'ab') as f:                      # a file of another size
        f.write(b'\0' * 8)
    with pytest.raises(ValueError, match='floats'):
        arch.RegistrationNetWeights.load(str(tmp_path / 'view0'), cfg)


def test_config_from_gdnconf():
    # the keys of the reference's experiments/sawyer/registration_experiments/gdnconf.py
    conf = {'batch_size': 1, 'ch_mult': 4, 'orig_size': [96, 128], 'normalization': 'None', 'sequence_length': 30,
            'pretrained_model': ['/models/gdn/view0', '/models/gdn/view1'], 'fwd_bwd': '', 'flow_penal': 0.1,
            'occlusion_handling': 0.1}
    cfg, paths = arch.config_from_gdnconf(conf)
    assert (cfg.height, cfg.width, cfg.ch_mult) == (96, 128, 4)
    assert paths == ['/models/gdn/view0', '/models/gdn/view1']
    with pytest.raises(ValueError, match='normalization'):
        arch.config_from_gdnconf(dict(conf, normalization='in'))


def test_restatement_blocks_against_naive_loops():
    rs = np.random.RandomState(0)
    x = rs.normal(size=(2, 6, 8, 5))
    w3, b3 = rs.normal(size=(3, 3, 5, 4)), rs.normal(size=(4,))
    w5, b5 = rs.normal(size=(5, 5, 5, 2)), rs.normal(size=(2,))
    t = lambda a: torch.from_numpy(a)
    np.testing.assert_allclose(ora.conv_block(t(x), t(w3), t(b3)).numpy(), ora.naive_conv_block(x, w3, b3), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(ora.pool_block(t(x)).numpy(), ora.naive_pool_block(x))
    np.testing.assert_allclose(ora.upsample_block(t(x)).numpy(), ora.naive_upsample_block(x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(ora.conv_block(t(x), t(w5), t(b5), relu=False).numpy(),
                               ora.naive_conv_block(x, w5, b5, relu=False), rtol=0, atol=1e-12)
    assert ora.naive_conv_block(x, w3, b3).min() == 0 and ora.naive_conv_block(x, w5, b5, relu=False).min() < 0
    # an interior output of the up-sampling is the bilinear mix of its four nearest inputs
    up = ora.naive_upsample_block(x)
    np.testing.assert_allclose(up[:, 3, 5], 0.5625 * x[:, 1, 2] + 0.1875 * x[:, 2, 2] + 0.1875 * x[:, 1, 3] + 0.0625 * x[:, 2, 3],
                               rtol=1e-13)
    # float32 against float64: the whole chain, one view
    cfg = arch.RegistrationNetConfig(16, 24, 1)
    wts = arch.RegistrationNetWeights.random(cfg, seed=1)
    cur, ref = (rs.uniform(0, 1, (1, 16, 24, 3)).astype(np.float32) for _ in range(2))
    f64, f32 = ora.forward(wts, cur, ref, torch.float64), ora.forward(wts, cur, ref, torch.float32)
    assert f64.shape == (1, 16, 24, 2) and f64.dtype == np.float64 and f32.dtype == np.float32
    assert 0 < np.abs(f32 - f64).max() / np.abs(f64).max() < 1e-5
    # the whole chain block by block in naive loops
    x = np.concatenate([cur, ref], -1)
    for name in ('d1', 'd2', 'd3'):
        x = ora.naive_pool_block(ora.naive_conv_block(x, wts.tensors[name + '/w'], wts.tensors[name + '/b']))
    for name in ('u1', 'u2', 'u3'):
        x = ora.naive_upsample_block(ora.naive_conv_block(x, wts.tensors[name + '/w'], wts.tensors[name + '/b']))
    np.testing.assert_allclose(ora.naive_conv_block(x, wts.tensors['flow/w'], wts.tensors['flow/b'], relu=False), f64,
                               rtol=0, atol=1e-12)


@pytest.mark.parametrize('H,W,m,ncam', [(32, 32, 1, 2), (48, 64, 2, 1)])
def test_host_net_equals_the_restatement(H, W, m, ncam, tmp_path):
    hp = dict(image_height=H, image_width=W, ncam=ncam, ch_mult=m, seed=7, bias_scale=0.1)
    net = HostRegistrationNet('', hp).restore()
    rs = np.random.RandomState(H)
    cur, ref = (rs.uniform(0, 1, (2, ncam, H, W, 3)).astype(np.float32) for _ in range(2))
    flow = net.flow(cur, ref)
    want64 = ora.forward_views(net.weights, cur, ref, torch.float64)
    assert flow.shape == (2, ncam, H, W, 2) and flow.dtype == np.float32
    np.testing.assert_allclose(flow, want64, rtol=0, atol=2e-5 * np.abs(want64).max())
    np.testing.assert_allclose(flow, ora.forward_views(net.weights, cur, ref, torch.float32), rtol=0,
                               atol=1e-6 * np.abs(want64).max())
    assert np.abs(want64).max() > 0.1                                   # the random net moves pixels
    # a pair's flow depends on that pair alone (PyTorch's CPU convolutions pick their blocking by batch size: no bit claim)
    np.testing.assert_allclose(net.flow(cur[1:], ref[1:])[0], flow[1], rtol=0, atol=2e-5 * np.abs(want64).max())
    # from files: the same network; as a plug-in: (warped, flow, warp_pts) of one pair
    arch.save_registration_weights(net.weights, str(tmp_path))
    np.testing.assert_array_equal(HostRegistrationNet(str(tmp_path), hp).restore().flow(cur, ref), flow)
    per_view = [str(tmp_path / ('view%d' % v)) for v in range(ncam)]
    np.testing.assert_array_equal(HostRegistrationNet(per_view, hp).restore().flow(cur, ref), flow)
    warped, fl, pts = net(cur[0], ref[0])
    np.testing.assert_allclose(fl, flow[0], rtol=0, atol=2e-5 * np.abs(want64).max())
    want_warped, want_pts = oracle_reg.bilinear_warp_loops(cur[0], fl)
    np.testing.assert_array_equal(warped, want_warped)
    np.testing.assert_array_equal(pts, want_pts)
    with pytest.raises(ValueError):
        net.flow(cur[:, :, :-8], ref[:, :, :-8])
    with pytest.raises(ValueError):
        HostRegistrationNet('', hp).flow(cur, ref)                      # before restore()
    with pytest.raises(ValueError):
        HostRegistrationNet(net.weights[:1] * (ncam + 1), hp).restore()


def test_bilinear_warp_equals_the_loop_oracle_bit_for_bit():
    rs = np.random.RandomState(2)
    ncam, H, W = 2, 24, 32
    cur = rs.uniform(0, 1, (ncam, H, W, 3)).astype(np.float32)
    flow = rs.normal(0, 3.0, (ncam, H, W, 2)).astype(np.float32)
    flow[0, :3, :3] = -9.0                              # left of / above the frame: clamped
    flow[-1, -3:, -3:] = 11.0                           # right of / below
    flow[0, 5, 5] = (0.0, 0.0)
    flow[1, 6, 7] = (0.5, -0.25)
    flow[1, 0, :] = (100.0, -100.0)
    warped, pts = bilinear_warp(cur, flow)
    want_warped, want_pts = oracle_reg.bilinear_warp_loops(cur, flow)
    assert warped.dtype == np.float32 and pts.dtype == np.float32
    np.testing.assert_array_equal(pts, want_pts)
    np.testing.assert_array_equal(warped, want_warped)


def test_library_weight_count_and_refusals():
    _lib.build_library()
    lib = _lib.load_library()
    for H, W, m in ((64, 64, 4), (48, 64, 1), (128, 128, 2)):
        c = _lib.VfRegnetConfig(H, W, 2, m, 2, 0)
        assert lib.vf_regnet_weight_count(ctypes.byref(c)) == arch.RegistrationNetConfig(H, W, m).n_floats()
    for bad, msg in ((_lib.VfRegnetConfig(60, 64, 1, 1, 2, 0), b'multiples of 8'),
                     (_lib.VfRegnetConfig(64, 136, 1, 1, 2, 0), b'at most 128'),
                     (_lib.VfRegnetConfig(64, 64, 1, 3, 2, 0), b'ch_mult'),
                     (_lib.VfRegnetConfig(64, 64, 9, 1, 2, 0), b'ncam'),
                     (_lib.VfRegnetConfig(64, 64, 1, 1, 0, 0), b'max_pairs')):
        assert lib.vf_regnet_weight_count(ctypes.byref(bad)) == 0
        assert msg in lib.vf_last_error()
    assert lib.vf_regnet_flow(None, None, None, 1, None, None) != 0 and b'null' in lib.vf_last_error()
    assert lib.vf_regnet_destroy(None) == 0


def test_hip_net_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from visual_foresight_amd.video_prediction.registration_net import HipRegistrationNet
    with pytest.raises(_lib.VfError):
        HipRegistrationNet('', {'image_height': 64, 'image_width': 64})


def test_controller_plans_with_the_host_net_as_warper():
    H = W = 32
    T, ncam = 5, 2
    fake = make_fake_predictor_class(T, H, W, ncam=ncam)
    fake.n_cam = ncam
    net = HostRegistrationNet('', dict(image_height=H, image_width=W, ncam=ncam, ch_mult=1, seed=3)).restore()
    pol = {'predictor_class': fake, 'verbose': False, 'rejection_sampling': False, 'repeat': 1, 'num_samples': 20,
           'designated_pixel_count': 2, 'registration_warper': net, 'iterations': 2, 'trade_off_reg': True,
           'register_region': True}
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W, 'ncam': ncam}
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = RegisterGtruthController(ag, pol, 0, 1)
        ctrl.reset()
    rs = np.random.RandomState(0)
    images = rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8)
    goal_image = rs.uniform(0, 1, (1, ncam, H, W, 3)).astype(np.float32)
    states = rs.normal(size=(2, 5))
    np.random.seed(4)
    for t in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            out = ctrl.act(goal_image=goal_image, t=t, i_tr=0, desig_pix=[[10, 12], [20, 8]], goal_pix=[[5, 6], [25, 20]],
                           images=images[:t + 1], state=states[:t + 1])
    w = out['plan_stat']['tradeoff']
    assert w.shape == (ncam, 2) and np.isclose(w.sum(), 1.0) and np.all(w > 0)
    # the tracked pixels are the window medians of the net's own warp points
    cur = images[-1].astype(np.float32) / 255.
    start = images[0].astype(np.float32) / 255.
    _, _, pts = net(cur, start)
    win = pts[0, 8:13, 10:15]
    np.testing.assert_array_equal(ctrl._desig_pix[0, 0], (np.median(win[..., 1]), np.median(win[..., 0])))
    assert out['actions'].shape == (4,)
