"""Plan visualisation on the host: the message stream and page against the golden minted from the reference
(``tools/make_golden_plan_page.py``), the colouring against naive loops and matplotlib, the controllers with a recording
worker, the file writer, and the CPU-checkable parts of ``vf_render_plans``."""
import contextlib
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest

from tests.helpers.fake_frame_predictor import make_fake_frame_predictor_class
from tests.helpers.fake_plan_predictor import make_fake_plan_predictor_class
from tests.helpers.fake_predictor import make_fake_predictor_class
from visual_foresight_amd import _lib
from visual_foresight_amd.policy.cem_controllers import GoalImController, PixelCostController
from visual_foresight_amd.policy.cem_controllers.visualizer import colormap, plan_page
from visual_foresight_amd.utils import png
from visual_foresight_amd.utils.plan_page_writer import PlanPageWriter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = {'adim': 4, 'sdim': 5}


@contextlib.contextmanager
def _quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


class RecordingWorker(object):
    def __init__(self, extensions=None):
        self.messages = []
        if extensions is not None:
            self.asset_extensions = extensions

    def put(self, message):
        self.messages.append(message)


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'plan_page.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, 'plan_page.npz'))


def _assert_stream_equals_golden(messages, golden):
    meta, arrays = golden
    assert [(m[0], m[1]) for m in messages] == [(g['kind'], g['path']) for g in meta['messages']]
    for got, want in zip(messages, meta['messages']):
        if want['kind'] == 'txt_file':
            assert plan_page.parse_plan_page(got[2]) == want['content']
        else:
            payload = np.asarray(got[2])
            assert payload.dtype == np.uint8
            np.testing.assert_array_equal(payload, arrays[want['payload']], err_msg=want['path'])


# ---------------------------------------------------------------------------------------- the stream and the page
def test_messages_reproduce_the_reference_stream(golden):
    meta, arrays = golden
    H, W, T, ncam, nd = (meta[k] for k in ('H', 'W', 'T', 'ncam', 'ndesig'))
    fake = make_fake_plan_predictor_class(T, H, W, ncam=ncam)('', {})
    one_hot = np.zeros((2, ncam, H, W, nd), np.float32)
    for c in range(ncam):
        for p in range(nd):
            one_hot[:, c, meta['desig'][c][p][0], meta['desig'][c][p][1], p] = 1.
    context = {'context_frames': arrays['images'], 'context_pixel_distributions': one_hot}
    scores = arrays['last_scores']
    best = scores.argsort()[:10]
    assert len(best) == 10 < meta['M']                          # ten of the twelve plans are drawn
    prediction = fake(context, {'actions': arrays['last_actions'][best]})
    rendered = colormap.render_prediction(prediction['predicted_frames'], prediction['predicted_pixel_distributions'])
    assert rendered['frames'].shape == (10, ncam, T, H, W, 3)
    assert rendered['distributions'].shape == (10, ncam, nd, T, H, W, 3)
    messages = plan_page.build_plan_messages(
        1, meta['last_itr'], arrays['images'][-1], scores[best], rendered['frames'], rendered['distributions'],
        desig_pix=meta['desig'], goal_pix=meta['goal'], img_height=meta['policy']['verbose_img_height'])
    assert len(messages) == ncam + 10 * ncam * nd + 10 * ncam + 1
    _assert_stream_equals_golden(messages, golden)
    content = plan_page.parse_plan_page(messages[-1][2])
    assert content['heading'] == 'Visual MPC' and content['image_height'] == 96
    assert [r[0] for r in content['rows']] == ['cam_0_start', 'cam_1_start', 'cam_0_desig_0', 'cam_0_desig_1',
                                               'cam_1_desig_0', 'cam_1_desig_1', 'cam_0_pred_images',
                                               'cam_1_pred_images', 'scores']
    assert content['columns'] == ['traj_%d' % i for i in range(10)]


def test_controller_reproduces_the_reference_stream(golden):
    """The whole verbose planning call - sampler, host scoring, elite choice, rendering, messages - on the predictor and
    seeds the reference ran with."""
    meta, arrays = golden
    H, W, T, ncam = meta['H'], meta['W'], meta['T'], meta['ncam']
    fake = make_fake_plan_predictor_class(T, H, W, ncam=ncam)
    with _quiet():
        ctrl = PixelCostController(dict(AG, image_height=H, image_width=W), dict(meta['policy'], predictor_class=fake), 0, 1)
        ctrl.reset()
    worker = RecordingWorker()
    np.random.seed(meta['seed'])
    outs = []
    for t in range(2):
        with _quiet():
            outs.append(ctrl.act(t=t, i_tr=0, desig_pix=meta['desig'], goal_pix=meta['goal'],
                                 images=arrays['images'][:t + 1], state=arrays['states'][:t + 1], verbose_worker=worker))
    np.testing.assert_array_equal(outs[0]['actions'], arrays['action_t0'])
    np.testing.assert_array_equal(outs[1]['actions'], arrays['action_t1'])
    np.testing.assert_array_equal(ctrl.visualize_indices, arrays['last_scores'].argsort()[:10])
    _assert_stream_equals_golden(worker.messages, golden)


def test_marker_is_the_pixel_and_its_four_neighbours_clipped():
    img = np.zeros((5, 6, 3), np.uint8)
    plan_page.draw_marker(img, 2, 3, (255, 0, 0))
    assert sorted(zip(*np.nonzero(img[:, :, 0]))) == [(1, 3), (2, 2), (2, 3), (2, 4), (3, 3)]
    corner = plan_page.mark_start_image(np.zeros((5, 6, 3), np.uint8), [[0, 0]], [[4, 5]])
    assert sorted(zip(*np.nonzero(corner[:, :, 0]))) == [(0, 0), (0, 1), (1, 0)]            # red, clipped
    assert sorted(zip(*np.nonzero(corner[:, :, 2]))) == [(3, 5), (4, 4), (4, 5)]            # blue, clipped
    both = plan_page.mark_start_image(np.zeros((5, 6, 3), np.uint8), [[2, 2]], [[2, 3]])
    assert tuple(both[2, 2]) == (0, 0, 255) and tuple(both[2, 3]) == (0, 0, 255)            # the goal is drawn second
    assert tuple(both[1, 2]) == (255, 0, 0)
    outside = plan_page.mark_start_image(np.zeros((5, 6, 3), np.uint8), [[-3, 9]], [[7, -2]])
    assert not outside.any()


def test_workers_extensions_name_the_files():
    start = np.zeros((1, 8, 8, 3), np.uint8)
    frames = np.zeros((2, 1, 3, 8, 8, 3), np.uint8)
    ref = plan_page.build_plan_messages(4, 2, start, [0.5, 0.75], frames)
    assert [m[1] for m in ref] == ['planning_4_itr_2/assets/cam_0_start.jpg',
                                   'planning_4_itr_2/assets/cam_0_pred_images_0.gif',
                                   'planning_4_itr_2/assets/cam_0_pred_images_1.gif', 'planning_4_itr_2/plan.html']
    assert plan_page.asset_extensions(RecordingWorker()) == ('gif', 'jpg')
    assert plan_page.asset_extensions(PlanPageWriter()) == ('png', 'png')
    own = plan_page.build_plan_messages(4, 2, start, [0.5, 0.75], frames, extensions=('png', 'png'))
    rows = dict(plan_page.parse_plan_page(own[-1][2])['rows'])
    assert rows['cam_0_pred_images'] == ['assets/cam_0_pred_images_0.png', 'assets/cam_0_pred_images_1.png']
    assert rows['scores'] == ['0.5', '0.75']
    with pytest.raises(ValueError):
        plan_page.render_plan_page(0, 0, [('a', [1, 2]), ('b', [1])])


# ---------------------------------------------------------------------------------------- the colouring
def test_byte_table(golden):
    lut = colormap.VIRIDIS_U8
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    np.testing.assert_array_equal(lut, golden[1]['lut8'])


def test_byte_table_is_matplotlibs_viridis():
    pytest.importorskip('matplotlib')
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    np.testing.assert_array_equal(colormap.VIRIDIS_U8, (np.array(plt.cm.viridis.colors) * 255).astype(np.uint8))
    rs = np.random.RandomState(2)
    for i in range(20):
        dist = (rs.uniform(0, 1, (8, 12)) ** (1 + i % 5)).astype(np.float32)
        want = (np.squeeze(plt.cm.viridis(dist / (np.amax(dist) + 1e-6))[:, :, :3]) * 255).astype(np.uint8)
        np.testing.assert_array_equal(colormap.render_distribution_planes(dist), want)


def _naive_plane(plane, lut):
    H, W = plane.shape
    mx = np.float32(0)
    for r in range(H):
        for c in range(W):
            mx = max(mx, plane[r, c])
    denom = np.float32(mx + np.float32(1e-6))
    out = np.zeros((H, W, 3), np.uint8)
    for r in range(H):
        for c in range(W):
            q = np.float32(plane[r, c] / denom)
            out[r, c] = lut[min(int(np.float32(q * np.float32(256.))), 255)]
    return out


def test_render_distribution_planes_against_a_naive_loop():
    rs = np.random.RandomState(4)
    planes = rs.uniform(0, 1, (5, 8, 16)).astype(np.float32)
    planes[1] = 0.
    planes[1, 3, 5] = 1.                                        # one-hot
    planes[2] *= 0.3
    planes[2, -1, -1] = 0.9                                     # the maximum sits in the last pixel
    planes[3] = 0.                                              # all zero: every pixel is table row 0
    planes[4] /= planes[4].sum()                                # a normalised distribution
    lut = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    for table in (None, lut):
        got = colormap.render_distribution_planes(planes, table)
        assert got.dtype == np.uint8 and got.shape == (5, 8, 16, 3)
        for i in range(5):
            np.testing.assert_array_equal(got[i], _naive_plane(planes[i], colormap.check_lut(table)), err_msg=str(i))
    one_hot = colormap.render_distribution_planes(planes[1])
    assert tuple(one_hot[3, 5]) == tuple(colormap.VIRIDIS_U8[255]) and tuple(one_hot[0, 0]) == tuple(colormap.VIRIDIS_U8[0])
    assert tuple(colormap.render_distribution_planes(planes[2])[-1, -1]) == tuple(colormap.VIRIDIS_U8[255])
    # planes of a stack are coloured independently
    np.testing.assert_array_equal(colormap.render_distribution_planes(planes.reshape(5, 1, 8, 16))[:, 0],
                                  colormap.render_distribution_planes(planes))
    with pytest.raises(ValueError):
        colormap.render_distribution_planes(planes, lut[:100])


def test_render_frames_truncates():
    f = np.array([0., 0.5, 254.9 / 255., 1., 0.003921], np.float32)
    np.testing.assert_array_equal(colormap.render_frames(f), (f * 255).astype(np.uint8))
    assert colormap.render_frames(f).tolist() == [0, 127, 254, 255, 0]
    frames = np.random.RandomState(0).uniform(0, 1, (2, 3, 2, 4, 4, 3)).astype(np.float32)
    distrib = np.random.RandomState(1).uniform(0, 1, (2, 3, 2, 4, 4, 2)).astype(np.float32)
    out = colormap.render_prediction(frames, distrib)
    np.testing.assert_array_equal(out['frames'][1, 0, 2], (frames[1, 2, 0] * 255).astype(np.uint8))
    np.testing.assert_array_equal(out['distributions'][1, 0, 1, 2], _naive_plane(distrib[1, 2, 0, :, :, 1], colormap.VIRIDIS_U8))
    assert list(colormap.render_prediction(frames)) == ['frames']


# ---------------------------------------------------------------------------------------- the controllers
def _pixel_controller(worker_policy, ncam=1):
    fake = make_fake_plan_predictor_class(3, 16, 16, ncam=ncam)
    pol = dict(dict(num_samples=24, nactions=3, repeat=1, rejection_sampling=False, predictor_class=fake), **worker_policy)
    with _quiet():
        ctrl = PixelCostController(dict(AG, image_height=16, image_width=16), pol, 0, 1)
        ctrl.reset()
    return ctrl


def _run(ctrl, worker, seed=3, **extra):
    rs = np.random.RandomState(seed)
    ncam = ctrl._n_cam
    images = rs.randint(0, 256, (2, ncam, 16, 16, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    np.random.seed(seed)
    out = None
    for t in range(2):
        with _quiet():
            out = ctrl.act(t=t, i_tr=0, images=images[:t + 1], state=states[:t + 1], verbose_worker=worker, **extra)
    return out, images


def test_pixel_cost_controller_puts_the_page():
    pix = dict(desig_pix=[[4, 5]], goal_pix=[[10, 11]])
    worker = RecordingWorker()
    ctrl = _pixel_controller({})
    out, images = _run(ctrl, worker, **pix)
    scores = out['plan_stat']['scores_itr2']
    best = scores.argsort()[:10]
    np.testing.assert_array_equal(ctrl.visualize_indices, best)
    kinds = [m[0] for m in worker.messages]
    assert kinds == ['img'] + ['mov'] * 20 + ['txt_file']                      # only the last iteration draws a page
    assert all(m[1].startswith('planning_1_itr_2/') for m in worker.messages)
    np.testing.assert_array_equal(worker.messages[0][2], plan_page.mark_start_image(images[-1, 0], [[4, 5]], [[10, 11]]))
    seen = ctrl.predictor.actions_seen
    assert len(seen) == 4                                       # three iterations + the ten shown plans, rolled for the page
    np.testing.assert_array_equal(seen[3], seen[2][best])
    prediction = ctrl.predictor({'context_frames': images, 'context_pixel_distributions': ctrl._switch_on_pix(ctrl._desig_pix)},
                                {'actions': seen[2][best]})
    want = colormap.render_prediction(prediction['predicted_frames'], prediction['predicted_pixel_distributions'])
    for k in range(10):
        assert worker.messages[1 + k][1] == 'planning_1_itr_2/assets/cam_0_desig_0_%d.gif' % k
        np.testing.assert_array_equal(worker.messages[1 + k][2], want['distributions'][k, 0, 0])
        assert worker.messages[11 + k][1] == 'planning_1_itr_2/assets/cam_0_pred_images_%d.gif' % k
        np.testing.assert_array_equal(worker.messages[11 + k][2], want['frames'][k, 0])
        assert worker.messages[11 + k][2].shape == (3, 16, 16, 3) and worker.messages[11 + k][2].dtype == np.uint8
    rows = dict(plan_page.parse_plan_page(worker.messages[-1][2])['rows'])
    assert rows['scores'] == ['{}'.format(s) for s in scores[best]]
    # every iteration on request; a worker's own extensions
    every = RecordingWorker(('png', 'png'))
    _run(_pixel_controller({'verbose_every_iter': True}), every, **pix)
    assert [m[1] for m in every.messages if m[0] == 'txt_file'] == ['planning_1_itr_%d/plan.html' % i for i in range(3)]
    assert every.messages[0][1] == 'planning_1_itr_0/assets/cam_0_start.png'


def test_without_a_worker_nothing_changes():
    pix = dict(desig_pix=[[4, 5]], goal_pix=[[10, 11]])
    with_worker, _ = _run(_pixel_controller({}), RecordingWorker(), **pix)
    ctrl = _pixel_controller({})
    without, _ = _run(ctrl, None, **pix)
    np.testing.assert_array_equal(without['actions'], with_worker['actions'])
    for k, v in with_worker['plan_stat'].items():
        np.testing.assert_array_equal(without['plan_stat'][k], v)
    assert not hasattr(ctrl, 'visualize_indices')
    assert len(ctrl.predictor.actions_seen) == 3                                # no extra predictor call for a page
    silent = RecordingWorker()
    _run(_pixel_controller({'verbose': False}), silent, **pix)
    assert silent.messages == []


def test_predictor_with_render_plans_is_asked_for_the_bytes():
    base = make_fake_predictor_class(3, 16, 16)
    calls = []

    class Rendering(base):
        def render_plans(self, indices, lut=None, frames=True, distributions=True):
            calls.append((np.array(indices), frames, distributions))
            K = len(indices)
            return {'frames': np.full((K, 1, 3, 16, 16, 3), 7, np.uint8),
                    'distributions': np.full((K, 1, 1, 3, 16, 16, 3), 9, np.uint8)}

    pol = dict(num_samples=24, nactions=3, repeat=1, rejection_sampling=False, predictor_class=Rendering)
    with _quiet():
        ctrl = PixelCostController(dict(AG, image_height=16, image_width=16), pol, 0, 1)
        ctrl.reset()
    worker = RecordingWorker()
    n_before = len(base.calls)
    out, _ = _run(ctrl, worker, desig_pix=[[4, 5]], goal_pix=[[10, 11]])
    assert len(base.calls) - n_before == 3                                      # the three CEM iterations, nothing else
    assert len(calls) == 1 and calls[0][1:] == (True, True)
    np.testing.assert_array_equal(calls[0][0], out['plan_stat']['scores_itr2'].argsort()[:10])
    assert (worker.messages[1][2] == 9).all() and (worker.messages[11][2] == 7).all()


@pytest.mark.parametrize('ncam', [1, 2])
def test_goal_image_controller_puts_the_page(ncam):
    H, W = 16, 24
    fake = make_fake_frame_predictor_class(5, H, W, ncam=ncam)
    pol = dict(repeat=1, rejection_sampling=False, num_samples=40, predictor_class=fake)
    with _quiet():
        ctrl = GoalImController(dict(AG, image_height=H, image_width=W, ncam=ncam), pol, 0, 1)
        ctrl.reset()
    rs = np.random.RandomState(9)
    images = rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    goal = rs.randint(0, 256, (ncam, H, W, 3)).astype(np.uint8)
    results = []
    for worker in (RecordingWorker(), None):
        np.random.seed(0)
        with _quiet():
            ctrl.reset()
            ctrl.act(t=0, i_tr=0, images=images[:1], state=states[:1], goal_image=goal, verbose_worker=worker)
            results.append(ctrl.act(t=1, i_tr=0, images=images, state=states, goal_image=goal, verbose_worker=worker))
        if worker is not None:
            messages = worker.messages
    np.testing.assert_array_equal(results[0]['actions'], results[1]['actions'])
    scores = results[0]['plan_stat']['scores_itr2']
    best = scores.argsort()[:10]
    assert [m[0] for m in messages] == ['img'] * (2 * ncam) + ['mov'] * (10 * ncam) + ['txt_file']
    content = plan_page.parse_plan_page(messages[-1][2])
    assert [r[0] for r in content['rows']] == (['cam_%d_start' % c for c in range(ncam)] +
                                               ['cam_%d_goal' % c for c in range(ncam)] +
                                               ['cam_%d_pred_images' % c for c in range(ncam)] + ['scores'])
    assert content['iteration'] == '2' and content['t'] == '1' and content['image_height'] == 128
    for c in range(ncam):
        np.testing.assert_array_equal(messages[c][2], images[-1, c])            # no markers: no pixel is designated
        np.testing.assert_array_equal(messages[ncam + c][2], goal[c])
        assert messages[ncam + c][1] == 'planning_1_itr_2/assets/cam_%d_goal.jpg' % c
    frames = fake('', {})({'context_frames': images}, {'actions': ctrl.predictor.actions_seen[-1][best]})['predicted_frames']
    for c in range(ncam):
        for k in range(10):
            np.testing.assert_array_equal(messages[2 * ncam + c * 10 + k][2], colormap.render_frames(frames[k, :, c]))
    assert dict(content['rows'])['scores'] == ['{}'.format(s) for s in scores[best]]


# ---------------------------------------------------------------------------------------- the writer
def test_writer_puts_the_files_where_the_page_points(tmp_path, golden):
    meta, arrays = golden
    rs = np.random.RandomState(1)
    K, ncam, nd, T, H, W = 3, 2, 1, 4, 8, 16
    start = rs.randint(0, 256, (ncam, H, W, 3)).astype(np.uint8)
    frames = rs.randint(0, 256, (K, ncam, T, H, W, 3)).astype(np.uint8)
    distrib = rs.randint(0, 256, (K, ncam, nd, T, H, W, 3)).astype(np.uint8)
    writer = PlanPageWriter(str(tmp_path / 'unused'))
    writer.put(('path', str(tmp_path / 'run')))
    messages = plan_page.build_plan_messages(0, 1, start, [1., 2., 3.], frames, distrib, desig_pix=np.zeros((ncam, nd, 2), int),
                                             goal_pix=np.ones((ncam, nd, 2), int),
                                             extensions=plan_page.asset_extensions(writer))
    for m in messages:
        writer.put(m)
    writer.put(None)
    folder = tmp_path / 'run' / 'planning_0_itr_1'
    page = (folder / 'plan.html').read_text()
    assert page.endswith('</html>\n')
    content = plan_page.parse_plan_page(page)
    for name, cells in content['rows']:
        for k, cell in enumerate(cells):
            if name == 'scores':
                continue
            path = folder / cell
            assert path.is_file(), cell
            movie = png.read_apng(str(path))
            c = int(name.split('_')[1])
            if name.endswith('_start'):
                assert movie.shape[0] == 1
                np.testing.assert_array_equal(png.read_png(str(path)), messages[c][2])
            elif 'desig' in name:
                assert movie.shape[0] == T
                np.testing.assert_array_equal(movie, distrib[k, c, 0])
            else:
                assert movie.shape[0] == T
                np.testing.assert_array_equal(movie, frames[k, c])
                np.testing.assert_array_equal(png.read_png(str(path)), frames[k, c, 0])     # a still viewer: frame 0
    assert len(writer.written) == len(messages) and not (tmp_path / 'unused').exists()
    with pytest.raises(ValueError):
        writer.put(('sound', 'a.wav', None))
    with pytest.raises(ValueError):
        png.write_apng(str(tmp_path / 'x.png'), frames[0, 0, 0])


def test_animated_png_chunks(tmp_path):
    """acTL announces T frames, every frame has its fcTL, frames after the first travel as fdAT, sequence numbers run."""
    import struct
    frames = np.random.RandomState(0).randint(0, 256, (3, 4, 4, 3)).astype(np.uint8)
    path = str(tmp_path / 'm.png')
    png.write_apng(path, frames, fps=5)
    blob = open(path, 'rb').read()
    pos, tags, seqs = 8, [], []
    while pos < len(blob):
        n, tag = struct.unpack('>I4s', blob[pos:pos + 8])
        tags.append(tag)
        if tag in (b'fcTL', b'fdAT'):
            seqs.append(struct.unpack('>I', blob[pos + 8:pos + 12])[0])
        if tag == b'acTL':
            assert struct.unpack('>II', blob[pos + 8:pos + 16]) == (3, 0)
        if tag == b'fcTL':
            assert struct.unpack('>HH', blob[pos + 28:pos + 32]) == (1, 5)
        pos += 12 + n
    assert tags == [b'IHDR', b'acTL', b'fcTL', b'IDAT', b'fcTL', b'fdAT', b'fcTL', b'fdAT', b'IEND']
    assert seqs == list(range(5))
    np.testing.assert_array_equal(png.read_apng(path), frames)


def test_sim_writes_plan_pages(tmp_path):
    from visual_foresight_amd.sim.simulator import Sim, SyntheticAgent
    fake = make_fake_plan_predictor_class(3, 16, 16)
    config = {'agent': {'type': SyntheticAgent, 'T': 2, 'image_height': 16, 'image_width': 16,
                        'verbose_dir': str(tmp_path / 'verbose')},
              'policy': {'type': PixelCostController, 'num_samples': 12, 'nactions': 3, 'repeat': 1, 'iterations': 2,
                         'rejection_sampling': False, 'predictor_class': fake},
              'start_index': 0, 'end_index': 0, 'save_data': False}
    with _quiet():
        Sim(config).run()
    page = tmp_path / 'verbose' / 'traj0' / 'planning_1_itr_1' / 'plan.html'
    assert page.is_file()
    rows = dict(plan_page.parse_plan_page(page.read_text())['rows'])
    assert png.read_apng(str(page.parent / rows['cam_0_pred_images'][0])).shape == (3, 16, 16, 3)


# ---------------------------------------------------------------------------------------- the entry point
def test_vf_render_plans_is_exported_and_refuses_without_a_device():
    header = open(os.path.join(REPO, 'include', 'vf_hip.h')).read()
    m = re.search(r'\bint vf_render_plans\(([^;]*)\);', header)
    assert m, 'no prototype in the header'
    assert len(m.group(1).split(',')) == 7
    assert 'vf_render_plans' in _lib.EXPORTS
    assert re.search(r'#define VF_ABI_VERSION 7\b', header)
    _lib.build_library()
    lib = _lib.load_library()
    fn = lib.vf_render_plans
    P = ctypes.c_void_p
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [P, P, ctypes.c_int32, P, P, P, P]
    # refusals that need no device: nothing is dereferenced, no HIP call is made
    buf = (ctypes.c_uint8 * 16)()
    p = ctypes.cast(buf, P)
    assert fn(None, p, 1, p, p, p, None) == -1
    assert b'null' in lib.vf_last_error()
    with pytest.raises(_lib.VfError, match='null'):
        _lib.check(fn(None, None, 1, p, p, p, None))
    # the argument refusals come before the handle is read: any non-NULL pointer stands in for one
    stand_in = ctypes.cast((ctypes.c_uint8 * 4096)(), P)
    for args, word in (((stand_in, None, 1, p, p, p, None), b'null'),
                       ((stand_in, p, 1, p, None, None, None), b'both outputs'),
                       ((stand_in, p, 1, None, p, p, None), b'colour table'),
                       ((stand_in, p, 0, p, p, p, None), b'at least one'),
                       ((stand_in, p, -3, p, p, None, None), b'at least one')):
        assert fn(*args) == -1, word
        assert word in lib.vf_last_error(), lib.vf_last_error()
