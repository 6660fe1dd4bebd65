"""GPU parity of the action-inference network (``csrc/vf_inverse_model.h`` behind ``HipActionInference``): actions and the
hidden state of every step against the float64 restatement, bit-identity across calls / slots / instances / plan lengths,
``InvModelBaseController`` on the device against the same run on ``HostActionInference``, and the refusals."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.helpers import oracle_inverse_model as ora                                                   # noqa: E402
from visual_foresight_amd import _lib                                                                   # noqa: E402
from visual_foresight_amd.policy.inverse_models import InvModelBaseController                           # noqa: E402
from visual_foresight_amd.video_prediction.inverse_model import HipActionInference, HostActionInference  # noqa: E402
from visual_foresight_amd.video_prediction.inverse_model_arch import InverseModelConfig, InverseModelWeights  # noqa: E402

# The device may be this many times as far from float64 as the float32 restatement is on the same inputs (both are fp32
# chains that differ in addition order and in the last bits of expf / tanhf only; the rule and factor of HEAD_FACTOR in
# tests/test_gpu_learned_cost.py and of FLOW_FACTOR in tests/test_gpu_registration_net.py).
HEAD_FACTOR = 8.0
GUARD = 100.0       # the quantities the check is about are at least this many tolerances large


def _hp(H, W, adim, nc, na, max_batch=1, seed=0):
    return dict(image_height=H, image_width=W, adim=adim, n_context=nc, n_actions=na, max_batch=max_batch, seed=seed,
                bias_scale=0.1)


def _problems(seed, n, H, W, adim, nc):
    rs = np.random.RandomState(seed)
    img = (H, W, 3)
    return (rs.uniform(0, 1, (n,) + img).astype(np.float32), rs.uniform(0, 1, (n,) + img).astype(np.float32),
            rs.uniform(-1, 1, (n, nc, adim)).astype(np.float32), rs.uniform(0, 1, (n, nc) + img).astype(np.float32))


def check_against_float64(weights, inputs, dev_actions, dev_hidden, label):
    """The rule of test 1 on one call: prints both errors of the actions, h and c, asserts the guard and the factor.
    -> the tolerance of the actions."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    a64, h64 = ora.forward(weights, *inputs, dtype=torch.float64)
    a32, h32 = ora.forward(weights, *inputs, dtype=torch.float32)
    rows = [('actions', dev_actions, a32, a64), ('h', dev_hidden[:, :, 0], h32[:, :, 0], h64[:, :, 0]),
            ('c', dev_hidden[:, :, 1], h32[:, :, 1], h64[:, :, 1])]
    figures = []
    for name, dev, f32, f64 in rows:
        e_dev, e_32 = np.abs(dev - f64).max(), np.abs(f32 - f64).max()
        figures.append((name, e_dev, e_32))
        print('invmodel %s %s: device %.3g, float32 restatement %.3g from float64 (factor %.2f, allowed %.0f), largest |value| %.3g'
              % (label, name, e_dev, e_32, e_dev / e_32 if e_32 else np.inf, HEAD_FACTOR, np.abs(f64).max()))
    tol = HEAD_FACTOR * figures[0][2]
    # the guard: the check is about numbers that are large against its tolerance
    other_goal = np.ascontiguousarray(inputs[1][::-1, ::-1, ::-1])         # (another image: the goals flipped)
    a_other, _ = ora.forward(weights, inputs[0], other_goal, inputs[2], inputs[3], dtype=torch.float32)
    largest, goal_change = np.abs(a64).max(), np.abs(a_other - a32).max()
    print('invmodel %s guard: tolerance %.3g; largest |action| %.3g, change with the goal %.3g' % (label, tol, largest, goal_change))
    assert largest >= GUARD * tol and goal_change >= GUARD * tol
    if a64.shape[1] > 1:                                                    # (one action has no spread)
        spread = np.ptp(a64, axis=1).max()
        print('invmodel %s guard: spread over t %.3g' % (label, spread))
        assert spread >= GUARD * tol
    for name, e_dev, e_32 in figures:
        assert e_dev <= HEAD_FACTOR * e_32, name
    return tol


# H, W, adim, n_context, n_actions, n
CASES = [(16, 16, 4, 1, 1, 1),          # the smallest of every kind
         (48, 64, 4, 2, 15, 1),
         (64, 64, 4, 2, 15, 3),
         (64, 64, 5, 3, 7, 2),          # adim not a multiple of 4
         (32, 48, 1, 4, 32, 1),         # the longest recurrence, adim 1
         (96, 128, 8, 2, 30, 2)]        # the largest


@pytest.mark.parametrize('H,W,adim,nc,na,n', CASES)
def test_actions_and_hidden_state_against_the_float64_restatement(H, W, adim, nc, na, n):
    net = HipActionInference('', _hp(H, W, adim, nc, na, max_batch=n, seed=H + W + adim)).restore()
    inputs = _problems(H + na, n, H, W, adim, nc)
    actions, hidden = (t.cpu().numpy() for t in net.infer_device(*inputs, want_hidden=True))
    assert actions.shape == (n, na, adim) and actions.dtype == np.float32 and np.isfinite(actions).all()
    assert hidden.shape == (n, nc + na, 2, 128) and np.isfinite(hidden).all()
    np.testing.assert_array_equal(net.infer(*inputs), actions)              # d_hidden = NULL: the same actions
    check_against_float64(net.weights, inputs, actions, hidden, '%dx%d adim %d ctx %d T %d n %d' % (H, W, adim, nc, na, n))


def test_same_bits_alone_in_a_batch_again_elsewhere_and_for_a_shorter_plan():
    H, W, adim, nc, na, n = 64, 64, 4, 2, 15, 4
    net = HipActionInference('', _hp(H, W, adim, nc, na, max_batch=n, seed=3)).restore()
    inputs = _problems(9, n, H, W, adim, nc)
    full = net.infer(*inputs)
    assert len({full[i].tobytes() for i in range(n)}) == n                  # four different problems
    one = lambda i: tuple(x[i:i + 1] for x in inputs)
    for i in range(n):                                                      # alone
        np.testing.assert_array_equal(net.infer(*one(i))[0], full[i])
    rolled = tuple(np.ascontiguousarray(np.roll(x, 1, axis=0)) for x in inputs)     # slot 0 <-> the last slot, ...
    np.testing.assert_array_equal(net.infer(*rolled), np.roll(full, 1, axis=0))
    np.testing.assert_array_equal(net.infer(*inputs), full)                 # a second call
    twin = HipActionInference(net.weights, {'max_batch': 2}).restore()      # a second instance
    np.testing.assert_array_equal(twin.infer(*(x[2:] for x in inputs)), full[2:])
    # the reference's call and infer; device inputs are used where they lie
    np.testing.assert_array_equal(net(inputs[0][3], inputs[1][3], inputs[2][3:], inputs[3][3:]), full[3:])
    on_device = tuple(torch.from_numpy(x).to(net.device) for x in inputs)
    np.testing.assert_array_equal(net.infer_device(*on_device).cpu().numpy(), full)
    # a plan of 7 actions is the beginning of the plan of 15
    short_w = InverseModelWeights(InverseModelConfig(H, W, adim, nc, 7), net.weights.tensors)
    short = HipActionInference(short_w, {'max_batch': n}).restore()
    got = short.infer(*inputs)
    assert got.shape == (n, 7, adim)
    np.testing.assert_array_equal(got, full[:, :7])


def _recording(cls):
    class Recording(cls):
        def __call__(self, start, goal, ctx_actions, ctx_frames):
            out = super(Recording, self).__call__(start, goal, ctx_actions, ctx_frames)
            self.__dict__.setdefault('calls', []).append(
                (tuple(np.asarray(x, dtype=np.float32).copy() for x in (start, goal, ctx_actions, ctx_frames)), out.copy()))
            return out
    return Recording


def test_controller_on_the_device_against_the_host_network(tmp_path):
    """Eight steps of ``InvModelBaseController`` (two context steps, then a new plan every second step) with the device
    network and with the host network on the same weights, images and random stream.  Every plan of the device run obeys
    the rule of test 1 on the arguments its predictor was called with, and so does every plan of the host run.  The two
    runs see the same first call, whose plans therefore agree within the two tolerances; later calls differ in the context
    actions by no more than the earlier plans differed."""
    H, W, adim, steps = 64, 64, 4, 8
    cfg = InverseModelConfig(H, W, adim, n_context=2, n_actions=5)
    InverseModelWeights.random(cfg, seed=12).save(str(tmp_path))
    weights = InverseModelWeights.load(str(tmp_path))
    rs = np.random.RandomState(21)
    frames = rs.randint(0, 256, (steps, 1, H, W, 3)).astype(np.uint8)
    goal = rs.uniform(0, 1, (1, 1, H, W, 3))
    ag = {'adim': adim, 'sdim': 5, 'image_height': H, 'image_width': W}
    runs = []
    for cls in (_recording(HipActionInference), _recording(HostActionInference)):
        with contextlib.redirect_stdout(io.StringIO()):
            ctrl = InvModelBaseController(ag, {'predictor_class': cls, 'model_params_path': str(tmp_path), 'T': 5}, 0, 1)
            ctrl.reset()
            np.random.seed(5)
            trace = []
            for t in range(steps):
                out = ctrl.act(t=t, i_tr=0, images=frames[:t + 1], goal_image=goal)
                trace.append((np.asarray(out['actions']).copy(), ctrl.action_counter, len(ctrl.predictor.__dict__.get('calls', [])),
                              [None if f is None else f.copy() for f in ctrl.context_frames],
                              [None if a is None else np.asarray(a).copy() for a in ctrl.context_actions]))
        runs.append((ctrl, trace))
    (dev, dev_trace), (host, host_trace) = runs
    assert dev.predictor.cfg.as_dict() == host.predictor.cfg.as_dict() == cfg.as_dict()
    # bookkeeping: counters, which steps replanned, the context lists
    assert [t[1] for t in dev_trace] == [t[1] for t in host_trace] == [0, 0, 1, 2, 1, 2, 1, 2]
    assert [t[2] for t in dev_trace] == [t[2] for t in host_trace] == [0, 0, 1, 1, 2, 2, 3, 3]
    for d, h in zip(dev_trace, host_trace):
        assert len(d[3]) == len(h[3]) == len(d[4]) == len(h[4]) == 2
        # (after the first step the lists still hold one of the None entries reset() filled them with)
        assert [f is None for f in d[3]] == [f is None for f in h[3]] == [a is None for a in d[4]] == [a is None for a in h[4]]
        for a, b in zip(d[3], h[3]):
            if a is not None:
                np.testing.assert_array_equal(a, b)
    for t in (0, 1):                                                        # the random context actions
        np.testing.assert_array_equal(dev_trace[t][0], host_trace[t][0])
    assert len(dev.predictor.calls) == len(host.predictor.calls) == 3
    allowed = 0.0
    for k, ((d_in, d_out), (h_in, h_out)) in enumerate(zip(dev.predictor.calls, host.predictor.calls)):
        assert d_out.shape == h_out.shape == (1, 5, adim) and d_out.dtype == np.float32
        batched = (d_in[0][None], d_in[1][None], d_in[2], d_in[3])
        hidden = dev.predictor.infer_device(*batched, want_hidden=True)[1].cpu().numpy()
        tol = check_against_float64(weights, batched, d_out, hidden, 'controller plan %d' % k)
        for a, b in zip(d_in[:2] + d_in[3:], h_in[:2] + h_in[3:]):          # the images of the two runs are the same
            np.testing.assert_array_equal(a, b)
        # the host run is held to the same rule on its own arguments
        h_batched = (h_in[0][None], h_in[1][None], h_in[2], h_in[3])
        h_again, h_hidden = host.predictor.infer(*h_batched, want_hidden=True)
        np.testing.assert_array_equal(h_again, h_out)
        h_tol = check_against_float64(weights, h_batched, h_out, h_hidden, 'controller plan %d (host)' % k)
        # the two runs' context actions are the actions of their previous plans
        ctx_diff = np.abs(d_in[2] - h_in[2]).max()
        a64, _ = ora.forward(weights, *batched, dtype=torch.float64)
        h64, _ = ora.forward(weights, *h_batched, dtype=torch.float64)
        moved, diff = np.abs(a64 - h64).max(), np.abs(d_out - h_out).max()
        print('invmodel controller plan %d: context actions differ by %.3g -> float64 plans by %.3g; device - host %.3g '
              '(tolerances %.3g + %.3g)' % (k, ctx_diff, moved, diff, tol, h_tol))
        assert ctx_diff <= allowed
        if k == 0:                                                          # the same arguments: the plans agree
            assert moved == 0 and diff <= tol + h_tol
        allowed = diff                                                      # the next call's context holds these actions
    np.testing.assert_array_equal(dev_trace[2][0], dev.predictor.calls[0][1][0, 0])
    np.testing.assert_array_equal(dev_trace[7][0], dev.predictor.calls[2][1][0, 1])


def test_refusals():
    H, W, adim, nc, na = 32, 32, 4, 2, 3
    lib = _lib.load_library()
    hp = _hp(H, W, adim, nc, na, max_batch=2)
    net = HipActionInference('', hp)
    inputs = _problems(0, 3, H, W, adim, nc)
    with pytest.raises(ValueError, match='restore'):
        net.infer(*(x[:1] for x in inputs))
    net.restore()
    before = net.infer(*(x[:2] for x in inputs))
    with pytest.raises(_lib.VfError, match='max_batch'):
        net.infer(*inputs)                                                  # n = 3 > max_batch = 2
    # the Python size check: the reference does not resize either
    with pytest.raises(ValueError, match='32x32'):
        net(inputs[0][0, :16], inputs[1][0, :16], inputs[2][:1], inputs[3][:1, :, :16])
    with pytest.raises(ValueError, match='32x32'):
        net.infer(inputs[0][:1], inputs[1][:1, :, :16], inputs[2][:1], inputs[3][:1])
    with pytest.raises(ValueError):
        net.infer(inputs[0][:1], inputs[1][:1], inputs[2][:1, :1], inputs[3][:1])
    with pytest.raises(ValueError):
        net.infer(inputs[0][:2], inputs[1][:1], inputs[2][:1], inputs[3][:1])

    # through the ABI: refused on the host, nothing launched (the output keeps its filling)
    start, goal, ca, cf = (torch.from_numpy(x[:1]).to(net.device) for x in inputs)
    pad = torch.zeros(2 * H * W * 3 * nc + 4, dtype=torch.float32, device=net.device)
    out = torch.full((1, na, adim), 7.0, dtype=torch.float32, device=net.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(net.device).cuda_stream)
    assert pad.data_ptr() % 16 == 0
    S, G, CA, CF, O, off = start.data_ptr(), goal.data_ptr(), ca.data_ptr(), cf.data_ptr(), out.data_ptr(), pad.data_ptr() + 4
    infer = lib.vf_invmodel_infer
    for args, msg in (((None, S, G, CF, CA, 1, O), b'null'), ((net._handle, None, G, CF, CA, 1, O), b'null'),
                      ((net._handle, S, None, CF, CA, 1, O), b'null'), ((net._handle, S, G, None, CA, 1, O), b'null'),
                      ((net._handle, S, G, CF, None, 1, O), b'null'), ((net._handle, S, G, CF, CA, 1, None), b'null'),
                      ((net._handle, off, G, CF, CA, 1, O), b'16-byte aligned'), ((net._handle, S, off, CF, CA, 1, O), b'16-byte aligned'),
                      ((net._handle, S, G, off, CA, 1, O), b'16-byte aligned'),
                      ((net._handle, S, G, CF, CA, 0, O), b'max_batch'), ((net._handle, S, G, CF, CA, -1, O), b'max_batch'),
                      ((net._handle, S, G, CF, CA, 3, O), b'max_batch')):
        rc = infer(*(args + (None, stream)))
        assert rc == -1 and msg in lib.vf_last_error(), (args, lib.vf_last_error())
    c_cfg = _lib.VfInvModelConfig(H, W, adim, nc, na, 2, net.device.index, 1.0)
    empty = ctypes.c_void_p()
    assert lib.vf_invmodel_create(ctypes.byref(c_cfg), ctypes.byref(empty)) == 0
    assert infer(empty, S, G, CF, CA, 1, O, None, stream) == -1 and b'not loaded' in lib.vf_last_error()
    blob = net.weights.blob()
    assert lib.vf_invmodel_load_weights(empty, blob.ctypes.data_as(ctypes.c_void_p), blob.size - 1) == -1
    assert infer(empty, S, G, CF, CA, 1, O, None, stream) == -1 and b'not loaded' in lib.vf_last_error()
    assert lib.vf_invmodel_destroy(empty) == 0
    for bad in ((40, 32, 4, 2, 3, 1), (32, 144, 4, 2, 3, 1), (32, 32, 0, 2, 3, 1), (32, 32, 9, 2, 3, 1), (32, 32, 4, 0, 3, 1),
                (32, 32, 4, 5, 3, 1), (32, 32, 4, 2, 0, 1), (32, 32, 4, 2, 33, 1), (32, 32, 4, 2, 3, 0)):
        handle = ctypes.c_void_p()
        c_bad = _lib.VfInvModelConfig(*(bad + (net.device.index, 1.0)))
        assert lib.vf_invmodel_create(ctypes.byref(c_bad), ctypes.byref(handle)) == -1 and not handle.value, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    np.testing.assert_array_equal(net.infer(*(x[:2] for x in inputs)), before)      # the same bits afterwards
