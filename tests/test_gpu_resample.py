"""Area resampling on the device (``csrc/vf_resize.h`` behind ``vf_resize_area``) and what is wired to it: the kernel bit
for bit against the NumPy specification (``resample.area_resize_host``: int64 for uint8, the same-order float64 loop for
float32), a predictor fed camera-size context against one fed the host-shrunk context, ``vf_register_hw`` against
``vf_register`` and against ``registration.get_warp_err``, and the controllers that take the model's size from
``ag_params['model_image_height' / 'model_image_width']``."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from visual_foresight_amd import _lib                                                           # noqa: E402
from visual_foresight_amd.policy.cem_controllers import registration                            # noqa: E402
from visual_foresight_amd.video_prediction.resample import area_resize_device, area_resize_host  # noqa: E402

SIZES = [((96, 128), (48, 64)),         # factor 2
         ((240, 320), (48, 64)),        # factor 5
         ((480, 640), (48, 64)),        # factor 10
         ((192, 256), (96, 128)),       # factor 2, the inverse-model experiments' camera
         ((100, 136), (48, 64)),        # ratios 2.08 / 2.125: staged in LDS
         ((50, 70), (48, 64)),          # ratio below 2: footprints of at most 3
         ((9, 10), (8, 8))]


def _images(dtype, shape, seed):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        x = rs.randint(0, 256, shape).astype(np.uint8)
        x.reshape(-1)[::7] = 255            # runs of extremes: sums at the top of the range, exact ties
        x[..., :2, :, :] = 0
        return x
    # magnitudes over many binades, both signs: the float64 sum's order shows in the last float32 bit if it is wrong
    return (rs.normal(0, 1, shape) * np.exp(rs.uniform(-6, 6, shape))).astype(np.float32)


def _device(x):
    return torch.from_numpy(x).to('cuda:0')


@pytest.mark.parametrize('dtype', [np.uint8, np.float32], ids=['uint8', 'float32'])
@pytest.mark.parametrize('src,dst', SIZES, ids=['%dx%d-%dx%d' % (s + d) for s, d in SIZES])
def test_kernel_equals_the_specification_bit_for_bit(src, dst, dtype):
    for C in (1, 2, 3, 4):
        x = _images(dtype, (5,) + src + (C,), seed=C + src[0])
        want = area_resize_host(x, dst)
        got5 = area_resize_device(_device(x), dst).cpu().numpy()
        got1 = area_resize_device(_device(x[3:4]), dst).cpu().numpy()         # n = 1: image 3 alone
        assert got5.dtype == x.dtype and got5.shape == (5,) + dst + (C,)
        np.testing.assert_array_equal(got5, want)
        np.testing.assert_array_equal(got1[0], got5[3])                       # the same bits alone and as image 3 of 5
        assert got1.tobytes() == want[3:4].tobytes()                          # (bits, not values: -0.0, NaN payloads)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32], ids=['uint8', 'float32'])
@pytest.mark.parametrize('src,dst', [((96, 128), (48, 64)), ((100, 136), (48, 64)), ((9, 10), (8, 8))])
def test_a_base_offset_by_four_bytes_takes_the_unaligned_path(src, dst, dtype):
    """The 16-byte loads start at the first 16-byte boundary behind the base; in front of it and behind the last whole 16
    bytes the loads are scalar.  Offsets of 4 and 8 bytes (and, for bytes, 1 and 3) against the aligned call."""
    item = np.dtype(dtype).itemsize
    x = _images(dtype, (2,) + src + (3,), seed=9)
    want = area_resize_host(x, dst)
    for offset in (4, 8) + ((1, 3) if item == 1 else ()):
        flat = torch.zeros(x.size + 16 // item, dtype=torch.from_numpy(x).dtype, device='cuda:0')
        view = flat[offset // item: offset // item + x.size].view(x.shape)
        view.copy_(_device(x))
        assert view.data_ptr() % 16 == offset and view.is_contiguous()
        np.testing.assert_array_equal(area_resize_device(view, dst).cpu().numpy(), want)


def test_leading_axes_and_a_second_stream_give_the_same_bits():
    x = _images(np.uint8, (2, 3, 100, 136, 3), seed=1)           # [n_context, ncam, H, W, 3]: every leading axis is batch
    f = _images(np.float32, (2, 50, 70, 4), seed=2)
    dx, df = _device(x), _device(f)
    first = area_resize_device(dx, (48, 64)), area_resize_device(df, (48, 64))
    assert tuple(first[0].shape) == (2, 3, 48, 64, 3)
    side = torch.cuda.Stream(device='cuda:0')
    side.wait_stream(torch.cuda.current_stream('cuda:0'))
    with torch.cuda.stream(side):
        second = area_resize_device(dx, (48, 64), stream=side), area_resize_device(df, (48, 64), stream=side)
    side.synchronize()
    for a, b, host in zip(first, second, (x, f)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
        np.testing.assert_array_equal(a.cpu().numpy(), area_resize_host(host, (48, 64)))
    # equal sizes: a copy of the values (-0.0 comes back as +0.0, as in the specification), bit for bit the specification's
    z = np.array([-0.0, 0.0, -1.5, 3e-30, np.inf], np.float32).reshape(1, 5, 1)
    same = area_resize_device(_device(z), (1, 5)).cpu().numpy()
    assert same.tobytes() == area_resize_host(z, (1, 5)).tobytes() and not np.signbit(same[0, 0, 0])
    with pytest.raises(ValueError, match='shrinks only'):
        area_resize_device(dx, (101, 64))
    with pytest.raises(ValueError, match='contiguous'):
        area_resize_device(dx[..., ::2, :], (48, 32))
    with pytest.raises(ValueError, match='GPU'):
        area_resize_device(torch.from_numpy(x), (48, 64))


# ------------------------------------------------------------------ the predictor
T_PRED = 3


def _predictor(H, W, camera=None, nd=1, ncam=1, bs=4, T=T_PRED):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, ncam=ncam)
    if camera is not None:
        hp.update(camera_height=camera[0], camera_width=camera[1])
    return HipVPredEvaluation('', hp).restore()


@pytest.fixture(scope='module')
def small_predictor():
    return _predictor(16, 24)


@pytest.mark.parametrize('camera', [(32, 48), (40, 60)])
def test_rollout_from_a_camera_size_context(camera, small_predictor):
    """Model 16 x 24: the engine fed the camera's frames (shrunk on the device) against a second engine fed
    ``area_resize_host`` of them - frames, states, distributions and scores bit for bit."""
    from oracle import pixel_cost
    H, W, M = 16, 24, 4
    pred = _predictor(H, W, camera)
    assert pred.camera_size == camera and small_predictor.camera_size is None
    rs = np.random.RandomState(camera[0])
    frames = rs.randint(0, 256, (2, 1) + camera + (3,)).astype(np.uint8)
    ctx = {'context_frames': frames, 'context_actions': rs.normal(0, 0.05, (1, 4)),
           'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib([[[5, 7]]], 2, 1, H, W, 1)}
    small_ctx = dict(ctx, context_frames=area_resize_host(frames, (H, W)))
    actions = rs.normal(0, 0.1, (M, T_PRED, 4))
    goal = np.array([[[12, 3]]])
    got_scores, got_tasks = pred.score(ctx, {'actions': actions}, goal, finalweight=10.)
    got = pred(ctx, {'actions': actions})
    want_scores, want_tasks = small_predictor.score(small_ctx, {'actions': actions}, goal, finalweight=10.)
    want = small_predictor(small_ctx, {'actions': actions})
    assert got['predicted_frames'].shape == (M, T_PRED, 1, H, W, 3)           # everything downstream is at the model's size
    for k in ('predicted_frames', 'predicted_states', 'predicted_pixel_distributions'):
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(got_scores, want_scores)
    np.testing.assert_array_equal(got_tasks, want_tasks)
    assert np.isfinite(got_scores).all() and np.ptp(got_scores) > 0
    with pytest.raises(ValueError, match=r'camera size %d x %d.*model\s+size is 16 x 24' % camera):
        pred.score(small_ctx, {'actions': actions}, goal, finalweight=10.)


def test_camera_size_refusals():
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=16, image_width=24, sequence_length=5)
    with pytest.raises(ValueError, match='aspect'):
        HipVPredEvaluation('', dict(hp, camera_height=32, camera_width=40))
    with pytest.raises(ValueError, match='pair'):
        HipVPredEvaluation('', dict(hp, camera_height=32))
    with pytest.raises(ValueError, match='larger'):
        HipVPredEvaluation('', dict(hp, camera_height=8, camera_width=12))
    assert HipVPredEvaluation('', dict(hp, camera_height=16, camera_width=24)).camera_size is None


# ------------------------------------------------------------------ vf_register_hw
def _register_inputs(ncam, H, W, seed, ntask=5):
    from tests.helpers.flow_warper import synthetic_flow
    rs = np.random.RandomState(seed)
    cur, ref = (rs.uniform(0, 1, (ncam, H, W, 3)).astype(np.float32) for _ in range(2))
    flow = synthetic_flow(cur, ref, scale=3.0)
    flow[0, :3, :3] = -9.0                               # warp points left of / above the frame: clamped
    flow[-1, -3:, -3:] = 11.0
    pix = rs.randint(0, [H, W], (ncam, ntask, 2))
    pix[0, 0] = (0, 0)
    pix[0, 1] = (H - 1, W - 1)                           # windows clipped at both borders
    pix[-1, 2] = (1, W - 2)
    return cur, ref, flow, pix


def test_register_hw_at_the_handles_size_gives_vf_registers_bits():
    H, W, ncam = 32, 48, 2
    pred = _predictor(H, W, ncam=ncam)
    cur, ref, flow, pix = _register_inputs(ncam, H, W, seed=3)
    ntask = pix.shape[1]
    lib = _lib.load_library()
    d_cur, d_ref, d_fl = (torch.from_numpy(a).to(pred.device) for a in (cur, ref, flow))
    d_px = torch.from_numpy(pix.astype(np.int32)).to(pred.device)
    for region in (0, 2):
        for clip_sub in (1, 0):
            want = pred.register(cur, ref, flow, pix, region=region, clip_sub=clip_sub, want_warped=True)
            desig = torch.full((ncam, ntask, 2), -1.0, device=pred.device)
            err = torch.full((ncam, ntask), -1.0, device=pred.device)
            warped, pts = torch.zeros_like(d_cur), torch.zeros_like(d_fl)
            _lib.check(lib.vf_register_hw(pred._handle, H, W, d_cur.data_ptr(), d_ref.data_ptr(), d_fl.data_ptr(),
                                          d_px.data_ptr(), ntask, region, clip_sub, warped.data_ptr(), pts.data_ptr(),
                                          desig.data_ptr(), err.data_ptr(), pred._stream()))
            for got, w in zip((desig, err, warped, pts), want):
                assert got.cpu().numpy().astype(w.dtype).tobytes() == w.tobytes()


@pytest.mark.parametrize('region_on', [False, True], ids=['region0', 'region5'])
def test_register_hw_at_twice_the_handles_size_matches_get_warp_err(region_on):
    """Handle 48 x 64, registration at 96 x 128 (the reference's one registration experiment), against
    ``registration.get_warp_err`` on the same arrays; the tolerances of ``tests/test_gpu_registration.py``: tracked pixels
    equal (medians / flips of the same float32 warp points), errors to 2e-5 (float32 sums in another order)."""
    H, W, ncam = 48, 64, 2
    Hc, Wc = 2 * H, 2 * W
    pred = _predictor(H, W, camera=(Hc, Wc), ncam=ncam)
    cur, ref, flow, pix = _register_inputs(ncam, Hc, Wc, seed=5)
    pix[1, 3] = (Hc - 1, 0)                              # beyond the handle's own size on the row axis
    warped, pts = registration.bilinear_warp(cur, flow)
    region = 5 if region_on else 0                       # get_warp_err: 5 from 96 rows on
    for clip_sub, which in ((1, 'start'), (0, 'goal')):
        desig, err, got_warped, got_pts = pred.register(cur, ref, flow, pix, region=region, clip_sub=clip_sub,
                                                        want_warped=True)
        np.testing.assert_array_equal(got_pts, pts)
        np.testing.assert_allclose(got_warped, warped, rtol=0, atol=2e-7)
        assert desig.shape == (ncam, pix.shape[1], 2) and desig.max() > W       # camera coordinates
        for c in range(ncam):
            if which == 'start':
                eo, do = registration.get_warp_err(c, pix[c], pix[c], ref, ref, pts, None, warped, None, ['start'], region_on)
            else:
                eo, do = registration.get_warp_err(c, pix[c], pix[c], ref, ref, None, pts, None, warped, ['goal'], region_on)
            np.testing.assert_array_equal(desig[c], do[:, 0])
            np.testing.assert_allclose(err[c], eo[:, 0], rtol=2e-5)
    with pytest.raises(ValueError, match='model size 48 x 64 or the camera size 96 x 128'):
        pred.register(cur[:, :50], ref[:, :50], flow[:, :50], pix)


# ------------------------------------------------------------------ controllers
def test_register_controller_at_two_resolutions_device_against_host():
    """Camera 32 x 48, model 16 x 24, ``HipRegistrationNet`` at the camera's size: the device path (``vf_register_hw``) against
    ``registration_on_device=False`` (``get_warp_err`` at the camera's size) - tracked pixels and trade-off within the
    tolerances of ``tests/test_gpu_registration.py``, identical elites."""
    from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController
    from visual_foresight_amd.video_prediction.registration_net import HipRegistrationNet
    Hc, Wc, H, W = 32, 48, 16, 24
    ncam, T, M = 1, 3, 16
    net = HipRegistrationNet('', dict(image_height=Hc, image_width=Wc, ncam=ncam, ch_mult=1, max_pairs=2, seed=11,
                                      bias_scale=0.1)).restore()
    ag = {'adim': 4, 'sdim': 5, 'image_height': Hc, 'image_width': Wc, 'ncam': ncam,
          'model_image_height': H, 'model_image_width': W}
    base = {'nactions': T, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'num_samples': M,
            'designated_pixel_count': 2, 'registration_warper': net, 'iterations': 2, 'trade_off_reg': True,
            'register_region': True}
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (2, ncam, Hc, Wc, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal_image = rs.uniform(0, 1, (1, ncam, Hc, Wc, 3)).astype(np.float32)
    outs = []
    for on_device in (True, False):
        pol = dict(base) if on_device else dict(base, registration_on_device=False)
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = RegisterGtruthController(dict(ag), pol, 0, 1)
            assert (ctrl._img_height, ctrl._img_width) == (H, W) and ctrl.predictor.camera_size == (Hc, Wc)
            ctrl.reset()
            np.random.seed(0)
            kw = dict(goal_image=goal_image, i_tr=0, desig_pix=[[5, 7]], goal_pix=[[10, 20]])
            ctrl.act(t=0, images=frames[:1], state=states[:1], **kw)
            out = ctrl.act(t=1, images=frames, state=states, **kw)
        np.testing.assert_array_equal(ctrl.desig_pix_t0_med, [[[10, 14]]])      # (pix * 32 / 16).astype(int)
        np.testing.assert_array_equal(ctrl.goal_pix_med, [[[20, 40]]])
        outs.append((out, ctrl._best_indices.copy(), ctrl._desig_pix.copy()))
    (dev, dev_idx, dev_pix), (host, host_idx, host_pix) = outs
    assert dev_pix.shape == (ncam, 2, 2) and np.isfinite(dev_pix).all()
    assert (dev_pix[..., 0] <= H).all() and (dev_pix[..., 1] <= W).all()        # model coordinates
    np.testing.assert_array_equal(dev_pix, host_pix)
    np.testing.assert_allclose(dev['plan_stat']['tradeoff'], host['plan_stat']['tradeoff'], rtol=2e-5)
    np.testing.assert_array_equal(dev_idx, host_idx)
    np.testing.assert_array_equal(dev['actions'], host['actions'])


def test_inverse_model_shrinks_camera_size_images():
    """Camera 64 x 96, model 32 x 48: ``infer`` on the camera's images equals ``infer`` on host-shrunk images bit for bit."""
    from visual_foresight_amd.video_prediction.inverse_model import HipActionInference
    Hc, Wc, H, W, n, nctx = 64, 96, 32, 48, 2, 2
    hp = dict(image_height=H, image_width=W, adim=4, n_context=nctx, n_actions=5, max_batch=n, seed=3)
    model = HipActionInference('', dict(hp, camera_height=Hc, camera_width=Wc)).restore()
    rs = np.random.RandomState(6)
    start, goal = (rs.uniform(0, 1, (n, Hc, Wc, 3)).astype(np.float32) for _ in range(2))
    ctx_frames = rs.uniform(0, 1, (n, nctx, Hc, Wc, 3)).astype(np.float32)
    ctx_actions = rs.normal(0, 0.1, (n, nctx, 4)).astype(np.float32)
    got = model.infer(start, goal, ctx_actions, ctx_frames)
    want = model.infer(*(area_resize_host(x, (H, W)) for x in (start, goal)), ctx_actions, area_resize_host(ctx_frames, (H, W)))
    assert got.shape == (n, 5, 4) and np.isfinite(got).all() and np.ptp(got) > 0
    assert got.tobytes() == want.tobytes()
    plain = HipActionInference('', hp).restore(model.weights)
    np.testing.assert_array_equal(plain.infer(*(area_resize_host(x, (H, W)) for x in (start, goal)), ctx_actions,
                                              area_resize_host(ctx_frames, (H, W))), want)
    with pytest.raises(ValueError, match='not resized'):       # without the camera size a wrong-size image is refused as before
        plain.infer(start, goal, ctx_actions, ctx_frames)


def test_goal_image_controller_with_a_camera_size_goal():
    """``GoalImController`` at camera 32 x 48 / model 16 x 24: the scores of a planning call with the camera-size goal equal
    those with the host-shrunk goal bit for bit."""
    from visual_foresight_amd.policy.cem_controllers import GoalImController
    Hc, Wc, H, W = 32, 48, 16, 24
    ag = {'adim': 4, 'sdim': 5, 'image_height': Hc, 'image_width': Wc, 'model_image_height': H, 'model_image_width': W}
    pol = {'nactions': 3, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'num_samples': 8, 'iterations': 2}
    rs = np.random.RandomState(8)
    frames = rs.randint(0, 256, (2, 1, Hc, Wc, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal = rs.uniform(0, 1, (1, Hc, Wc, 3)).astype(np.float32)
    outs = []
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = GoalImController(dict(ag), dict(pol), 0, 1)
        for g in (goal, area_resize_host(goal, (H, W))):
            ctrl.reset()
            np.random.seed(0)
            ctrl.act(t=0, i_tr=0, images=frames[:1], state=states[:1], goal_image=g)
            out = ctrl.act(t=1, i_tr=0, images=frames, state=states, goal_image=g)
            outs.append((out['plan_stat']['scores_itr0'].copy(), out['plan_stat']['scores_itr1'].copy(), out['actions'].copy()))
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.ptp(outs[0][0]) > 0
