"""GPU parity of the registration network (``csrc/vf_registration_net.h`` behind ``HipRegistrationNet``): flows against the
float64 restatement, bit-identity across calls / slots / clones, registration straight from the device flow, a planning
call of ``RegisterGtruthController`` against the same call with ``HostRegistrationNet``, and the refusals."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import registration as oracle_reg                                                           # noqa: E402
from tests.helpers import oracle_registration_net as ora                                                # noqa: E402
from visual_foresight_amd import _lib                                                                   # noqa: E402
from visual_foresight_amd.video_prediction.registration_net import HipRegistrationNet, HostRegistrationNet   # noqa: E402

# The device may be this many times as far from float64 as the float32 restatement is on the same inputs (both are fp32
# chains that differ in addition order only; the rule and factor of HEAD_FACTOR in tests/test_gpu_learned_cost.py).
FLOW_FACTOR = 8.0


def _hp(H, W, m, ncam, max_pairs=2, seed=11):
    return dict(image_height=H, image_width=W, ncam=ncam, ch_mult=m, max_pairs=max_pairs, seed=seed, bias_scale=0.1)


def _pairs(seed, n, ncam, H, W):
    rs = np.random.RandomState(seed)
    return tuple(rs.uniform(0, 1, (n, ncam, H, W, 3)).astype(np.float32) for _ in range(2))


def flow_errors(weights, cur, ref, device_flow):
    """(device error, float32 restatement's error), each max |x - float64| / max |float64 flow|; and max |flow|."""
    f64 = ora.forward_views(weights, cur, ref, torch.float64)
    f32 = ora.forward_views(weights, cur, ref, torch.float32)
    scale = np.abs(f64).max()
    return np.abs(device_flow - f64).max() / scale, np.abs(f32 - f64).max() / scale, scale


@pytest.mark.parametrize('H,W,m,ncam,n', [(48, 64, 1, 1, 1), (48, 64, 4, 2, 2), (64, 64, 1, 2, 2), (64, 64, 4, 1, 1),
                                          (64, 64, 4, 2, 2), (64, 64, 2, 2, 2), (96, 128, 1, 2, 1), (96, 128, 4, 2, 2), (128, 128, 1, 1, 2),
                                          (128, 128, 4, 2, 1), (40, 56, 1, 2, 2)])
def test_flow_against_the_float64_restatement(H, W, m, ncam, n):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = HipRegistrationNet('', _hp(H, W, m, ncam)).restore()
    cur, ref = _pairs(H + W + m, n, ncam, H, W)
    got = net.flow(cur, ref)
    assert got.shape == (n, ncam, H, W, 2) and got.dtype == np.float32 and np.isfinite(got).all()
    dev, f32, scale = flow_errors(net.weights, cur, ref, got)
    print('regnet %dx%d m %d ncam %d n %d: device %.3g, float32 restatement %.3g of the largest |flow| %.3g px (factor %.2f, '
          'allowed %.0f)' % (H, W, m, ncam, n, dev, f32, scale, dev / f32, FLOW_FACTOR))
    assert scale > 0.5, 'the random network moves pixels'
    assert dev <= FLOW_FACTOR * f32


def test_same_bits_alone_in_a_batch_on_a_clone_and_on_the_host_copy():
    H, W, m, ncam = 64, 64, 4, 2
    net = HipRegistrationNet('', _hp(H, W, m, ncam)).restore()
    cur, ref = _pairs(5, 2, ncam, H, W)
    both = net.flow_device(cur, ref)
    np.testing.assert_array_equal(net.flow(cur, ref), both.cpu().numpy())
    both = both.cpu().numpy()
    for i in range(2):                                          # alone; and in the other slot
        np.testing.assert_array_equal(net.flow(cur[i:i + 1], ref[i:i + 1])[0], both[i])
    np.testing.assert_array_equal(net.flow(cur[::-1].copy(), ref[::-1].copy()), both[::-1])
    clone = net.clone_to(net.device)
    np.testing.assert_array_equal(clone.flow(cur, ref), both)
    # device inputs are used where they lie
    d_cur, d_ref = (torch.from_numpy(a).to(net.device) for a in (cur, ref))
    np.testing.assert_array_equal(net.flow_device(d_cur, d_ref).cpu().numpy(), both)
    # a narrower net (u3 has 16 channels in a 32-wide tile) and a non-square one
    small = HipRegistrationNet('', _hp(48, 64, 1, 1)).restore()
    c2, r2 = _pairs(6, 2, 1, 48, 64)
    np.testing.assert_array_equal(small.flow(c2[1:], r2[1:])[0], small.flow(c2, r2)[1])
    assert not np.array_equal(both[0, 0], both[0, 1])           # one weight set per view


def _predictor(H, W, ncam):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=1, run_batch_size=4, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=4, ncam=ncam)
    return HipVPredEvaluation('', hp).restore()


@pytest.mark.parametrize('H,W,ncam', [(64, 64, 2), (96, 128, 1)])
def test_registration_from_the_device_flow(H, W, ncam):
    pred = _predictor(H, W, ncam)
    net = HipRegistrationNet('', _hp(H, W, 1, ncam)).restore()
    cur, ref = _pairs(H, 2, ncam, H, W)
    flows = net.flow_device(cur, ref)
    rs = np.random.RandomState(1)
    pix = rs.randint(0, [H, W], (ncam, 5, 2))
    pix[0, 0] = (0, 0)
    pix[0, 1] = (H - 1, W - 1)
    for i in range(2):
        flow_np = flows[i].cpu().numpy()
        want_warped, want_pts = oracle_reg.bilinear_warp_loops(cur[i], flow_np)
        for region_on, clip_sub, which in ((True, 1, 'start'), (True, 0, 'goal'), (False, 1, 'start')):
            region = (5 if H >= 96 else 2) if region_on else 0
            dev = pred.register(torch.from_numpy(cur[i]).to(pred.device), torch.from_numpy(ref[i]).to(pred.device), flows[i],
                                pix, region=region, clip_sub=clip_sub, want_warped=True)
            host = pred.register(cur[i], ref[i], flow_np, pix, region=region, clip_sub=clip_sub, want_warped=True)
            mixed = pred.register(cur[i], ref[i], flows[i], pix, region=region, clip_sub=clip_sub)
            for a, b in zip(dev, host):
                np.testing.assert_array_equal(a, b)
            for a, b in zip(mixed, host):
                np.testing.assert_array_equal(a, b)
            desig, err, warped, pts = dev
            np.testing.assert_array_equal(pts, want_pts)
            np.testing.assert_allclose(warped, want_warped, rtol=0, atol=2e-7)
            for c in range(ncam):
                if which == 'start':
                    eo, do = oracle_reg.warp_err_loops(c, pix[c], pix[c], ref[i], ref[i], want_pts, None, want_warped, None,
                                                       ['start'], region_on)
                else:
                    eo, do = oracle_reg.warp_err_loops(c, pix[c], pix[c], ref[i], ref[i], None, want_pts, None, want_warped,
                                                       ['goal'], region_on)
                np.testing.assert_array_equal(desig[c], do[:, 0])
                np.testing.assert_allclose(err[c], eo[:, 0], rtol=2e-5)


# ------------------------------------------------------------------------------------------------------------- end to end
E2E = dict(H=64, W=64, ncam=2, m=4, net_seed=11, image_seed=4, desig_pix=[[20, 30], [40, 12]], goal_pix=[[10, 50], [33, 33]])
INT_MARGIN = 1e-3           # px: every tracked coordinate of the host run lies at least this far from an integer


def e2e_inputs():
    H, W, ncam = E2E['H'], E2E['W'], E2E['ncam']
    rs = np.random.RandomState(E2E['image_seed'])
    frames = rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, .1, (2, 5))
    goal_image = rs.uniform(0, 1, (1, ncam, H, W, 3)).astype(np.float32)
    return frames, states, goal_image


def distance_from_integers(x):
    return np.abs(x - np.round(x)).min()


def test_planning_call_matches_the_host_net():
    """``RegisterGtruthController`` on the engine with the device net against the same call with ``HostRegistrationNet`` on
    the same weights (both register on the device; only the source of the flow differs).

    Flow tolerance: the device is within FLOW_FACTOR x e32 of float64 (first test), the host net within about 1 x e32
    (it is the float32 restatement), so the two flows differ by at most delta = (FLOW_FACTOR + 1) * e32 * max |flow| px.
    Images lie in [0, 1], so a bilinear sample moves by at most 2 * delta (one delta per axis, slope <= 1), a squared
    photometric difference by at most 2 * 1 * 2 * delta, hence a window's warp error by 4 * delta, relatively
    4 * delta / err; on top of that vf_register's own 2e-5.  A trade-off weight (1 / err) / sum(1 / err) moves relatively by
    at most twice the largest relative change of an error.

    Figures (one MI355X; profiles/registration_net.txt): tracked coordinates of the host run lie >= 0.139 px from an
    integer (checked on the CPU when the seeds were chosen); delta 4.88e-5 px (e32 2.6e-6, max |flow| 2.09 px), smallest warp
    error 0.107 -> trade-off tolerance 3.69e-3, seen 5.4e-7; scores differ by at most 1.1e-6 in every iteration against gaps
    of 5.19e-4, 1.55e-5 and 6.53e-5 at the elite boundary."""
    from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W, ncam = E2E['H'], E2E['W'], E2E['ncam']
    hp = _hp(H, W, E2E['m'], ncam, seed=E2E['net_seed'])
    dev_net = HipRegistrationNet('', hp).restore()
    host_net = HostRegistrationNet(dev_net.weights, hp).restore()
    frames, states, goal_image = e2e_inputs()
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W, 'ncam': ncam}
    base = {'nactions': 3, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'num_samples': 48,
            'designated_pixel_count': 2, 'trade_off_reg': True, 'register_region': True}    # (['start', 'goal'], 3 iterations: defaults)
    outs = []
    for net in (dev_net, host_net):
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = RegisterGtruthController(dict(ag), dict(base, registration_warper=net), 0, 1)
            ctrl.reset()
            np.random.seed(0)
            kw = dict(goal_image=goal_image, i_tr=0, desig_pix=E2E['desig_pix'], goal_pix=E2E['goal_pix'])
            ctrl.act(t=0, images=frames[:1], state=states[:1], **kw)
            out = ctrl.act(t=1, images=frames, state=states, **kw)
        outs.append((out, ctrl._desig_pix.copy(), ctrl._elite_count()))
    (dev, dev_pix, K), (host, host_pix, _) = outs

    # the fixture's two properties, asserted on the host run
    dist = distance_from_integers(host_pix)
    print('regnet e2e: tracked coordinates of the host run lie >= %.3g px from an integer' % dist)
    assert dist >= INT_MARGIN, 'fixture seeds put a tracked coordinate on an integer boundary'
    np.testing.assert_array_equal(dev_pix.astype(int), host_pix.astype(int))

    cur = frames[-1].astype(np.float32) / 255.
    refs = np.stack([frames[0].astype(np.float32) / 255., goal_image[-1]])
    curs = np.broadcast_to(cur, refs.shape)
    _, e32, scale = flow_errors(dev_net.weights, curs, refs, host_net.flow(curs, refs))
    delta = (FLOW_FACTOR + 1) * e32 * scale
    err_min = host['plan_stat']['warperrs'].min()
    tol = 2 * (4 * delta / err_min + 2e-5)
    rel = np.abs(dev['plan_stat']['tradeoff'] / host['plan_stat']['tradeoff'] - 1).max()
    print('regnet e2e: flows differ by at most delta %.3g px (e32 %.3g, max |flow| %.3g), smallest warp error %.3g -> trade-off '
          'tolerance %.3g; seen %.3g' % (delta, e32, scale, err_min, tol, rel))
    assert rel <= tol
    for itr in range(3):
        s_dev, s_host = dev['plan_stat']['scores_itr%d' % itr], host['plan_stat']['scores_itr%d' % itr]
        srt = np.sort(s_host)
        diff, gap = np.abs(s_dev - s_host).max(), srt[K] - srt[K - 1]
        print('regnet e2e itr %d: max |device - host| score %.3g, host gap at the elite boundary %.3g' % (itr, diff, gap))
        assert gap > 4 * diff, 'fixture seeds give an ambiguous elite boundary'
        np.testing.assert_array_equal(np.sort(np.argsort(s_dev)[:K]), np.sort(np.argsort(s_host)[:K]))
    np.testing.assert_array_equal(dev['actions'], host['actions'])


def test_refusals():
    H, W, ncam = 64, 64, 1
    hp = _hp(H, W, 1, ncam)
    lib = _lib.load_library()
    net = HipRegistrationNet('', hp)
    cur, ref = _pairs(0, 3, ncam, H, W)
    with pytest.raises(_lib.VfError, match='not loaded'):
        net.flow(cur[:1], ref[:1])                              # before restore()
    net.restore()
    with pytest.raises(_lib.VfError, match='max_pairs'):
        net.flow(cur, ref)                                      # n = 3 > max_pairs = 2
    with pytest.raises(ValueError):
        net.flow(cur[:1, :, :32], ref[:1, :, :32])              # shape mismatch
    with pytest.raises(ValueError):
        net.flow(cur[:2], ref[:1])
    # a misaligned pointer through the ABI: refused on the host, nothing launched
    d_cur, d_ref = (torch.from_numpy(a[:1]).to(net.device) for a in (cur, ref))
    pad = torch.zeros(H * W * 3 + 4, dtype=torch.float32, device=net.device)
    out = torch.empty((1, ncam, H, W, 2), dtype=torch.float32, device=net.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(net.device).cuda_stream)
    assert pad.data_ptr() % 16 == 0
    rc = lib.vf_regnet_flow(net._handle, pad.data_ptr() + 4, d_ref.data_ptr(), 1, out.data_ptr(), stream)
    assert rc != 0 and b'16-byte aligned' in lib.vf_last_error()
    rc = lib.vf_regnet_flow(net._handle, d_cur.data_ptr(), None, 1, out.data_ptr(), stream)
    assert rc != 0 and b'null' in lib.vf_last_error()
    bad = _lib.VfRegnetConfig(64, 136, 1, 1, 2, 0)
    handle = ctypes.c_void_p()
    assert lib.vf_regnet_create(ctypes.byref(bad), ctypes.byref(handle)) != 0 and not handle.value
    torch.cuda.synchronize()
    np.testing.assert_array_equal(net.flow(cur[:1], ref[:1]), net.flow(cur[:2], ref[:2])[:1])     # still usable

    # a net on another device than the predictor: the controller refuses before anything runs
    from visual_foresight_amd.policy.cem_controllers import RegisterGtruthController
    if torch.cuda.device_count() > 1:
        other = net.clone_to(1)
    else:                                                       # one GPU: the same net claiming the next ordinal
        other = net
        other.device = torch.device('cuda', 1)
    ag = {'adim': 4, 'sdim': 5, 'image_height': H, 'image_width': W, 'ncam': ncam}
    pol = {'nactions': 3, 'repeat': 1, 'rejection_sampling': False, 'verbose': False, 'num_samples': 8,
           'designated_pixel_count': 2, 'iterations': 1, 'registration_warper': other}
    frames = np.random.RandomState(0).randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8)
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl = RegisterGtruthController(ag, pol, 0, 1)
        ctrl.reset()
        kw = dict(goal_image=np.zeros((1, ncam, H, W, 3), np.float32), i_tr=0, desig_pix=[[5, 5]], goal_pix=[[9, 9]])
        with pytest.raises(ValueError, match='registration net lives on'):
            ctrl.act(t=0, images=frames[:1], state=np.zeros((1, 5)), **kw)
            ctrl.act(t=1, images=frames, state=np.zeros((2, 5)), **kw)
    if torch.cuda.device_count() > 1:
        pred = _predictor(H, W, ncam)
        with pytest.raises(ValueError, match='registers on'):
            pred.register(cur[0], ref[0], other.flow_device(cur[:1], ref[:1])[0], [[[5, 5]]])
