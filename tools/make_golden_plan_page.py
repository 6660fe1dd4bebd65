#!/usr/bin/env python
"""Mint tests/golden/plan_page.{json,npz} from the REAL reference plan page.

Imports the reference's ``PixelCostController`` under ``tools/make_golden.py``'s stubs (that file is not edited), hands
it a recording queue as ``verbose_worker`` and ``tests/helpers/fake_plan_predictor.py`` as predictor (8 x 8 images,
T = 3, M = 12 samples, two views, two designated pixels: 10 of the 12 plans are drawn) and runs one verbose planning call.
The reference colours the distributions through the matplotlib installed here.  Two stand-ins:

* ``cv2.circle`` draws the marker ``visualizer/plan_page.py`` defines (the pixel and its four neighbours, clipped) - OpenCV
  is not part of this stack and the reference's own marker is not pinned;
* the reference hard-codes ``_n_cam = 1`` (``pixel_cost_controller.py:43``); it is set to the predictor's two views after
  construction, which is all its multi-view code paths need.

Recorded: the message list (kinds, paths, uint8 payloads), the byte table ``(viridis.colors * 255).astype(uint8)``, the
inputs a test needs to replay the call (observations, designated / goal pixels, seeds, the actions and scores of the
last iteration) and the page's CONTENT - heading, iteration, t, image height, column titles, ordered rows as name ->
cells - parsed out of the reference's page here.  The page text itself carries the reference's markup and is not
stored: the ``'txt_file'`` message keeps its kind and path, its payload is replaced by that content.

    python tools/make_golden_plan_page.py        # rewrites tests/golden/plan_page.{json,npz}
"""
import json
import os
import re
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as mg  # noqa: E402

from tests.helpers.fake_plan_predictor import make_fake_plan_predictor_class  # noqa: E402
from visual_foresight_amd.policy.cem_controllers.visualizer.plan_page import draw_marker  # noqa: E402

OUT = os.path.join(mg.REPO, 'tests', 'golden')

H = W = 8
T, M, NCAM, NDESIG = 3, 12, 2, 2
SEED = 4100
DESIG = [[[2, 3], [5, 5]], [[0, 7], [6, 1]]]      # [ncam][ndesig](row, col); the second view's touch the border
GOAL = [[[6, 6], [1, 2]], [[7, 0], [3, 3]]]
POLICY = dict(num_samples=M, iterations=2, nactions=T, repeat=1, rejection_sampling=False,
              designated_pixel_count=NDESIG, verbose_img_height=96)     # (verbose: the default, True)


class RecordingQueue(object):
    def __init__(self):
        self.messages = []

    def put(self, message):
        self.messages.append(message)


def circle_stub(img, centre, radius, colour, thickness):
    assert radius == 1 and thickness == -1
    draw_marker(img, centre[1], centre[0], colour)      # OpenCV points are (x, y) = (col, row)


def observations():
    rs = np.random.RandomState(SEED)
    images = rs.randint(0, 256, (2, NCAM, H, W, 3)).astype(np.uint8)
    states = rs.normal(0, 0.1, (2, 5))
    return images, states


def parse_reference_page(text):
    """The content of a page of the reference's ``fill_template`` (construct_html.py:1-74)."""
    content = {'heading': re.search(r'<h2>(.*?)</h2>', text).group(1).strip(), 'columns': [], 'rows': [],
               'image_height': None}
    m = re.search(r'Iter=(\S+), t=(\S+?)</p>', text)
    content['iteration'], content['t'] = m.group(1), m.group(2)
    for row in re.findall(r'<tr>(.*?)</tr>', text, re.S):
        titles = re.findall(r'<th>(.*?)</th>', row, re.S)
        if titles:
            content['columns'] = [c.strip() for c in titles if c.strip()]
            continue
        cells = [c.strip() for c in re.findall(r'<td>(.*?)</td>', row, re.S)]
        name = re.fullmatch(r'<b>(.*?)</b>', cells[0], re.S).group(1).strip()
        values = []
        for c in cells[1:]:
            img = re.fullmatch(r'<img src="(.*?)" height="(\d+)">', c)
            if img:
                heights = {content['image_height'], int(img.group(2))} - {None}
                assert len(heights) == 1
                content['image_height'] = heights.pop()
                values.append(img.group(1))
            else:
                values.append(c)
        content['rows'].append([name, values])
    return content


def main():
    mg.install_stubs()
    sys.modules['cv2'].circle = circle_stub
    from visual_mpc.policy.cem_controllers import PixelCostController
    import matplotlib.pyplot as plt
    import matplotlib

    fake = make_fake_plan_predictor_class(T, H, W, ncam=NCAM)
    mg.reference_predictor(fake)
    ag = dict(mg.AG, image_height=H, image_width=W)
    with mg.quiet():
        ctrl = PixelCostController(ag, dict(POLICY), 0, 1)
        ctrl._n_cam = NCAM
        ctrl.reset()
    images, states = observations()
    queue = RecordingQueue()
    np.random.seed(SEED)
    outs = []
    for t in range(2):
        with mg.quiet():
            outs.append(ctrl.act(t=t, i_tr=0, desig_pix=DESIG, goal_pix=GOAL, images=images[:t + 1],
                                 state=states[:t + 1], verbose_worker=queue))
    last_itr = POLICY['iterations'] - 1
    scores = np.array(outs[1]['plan_stat']['scores_itr%d' % last_itr])

    arrays = {'lut8': (np.array(plt.cm.viridis.colors) * 255).astype(np.uint8), 'images': images, 'states': states,
              'last_actions': fake.actions_seen[-1], 'last_scores': scores,
              'action_t0': np.array(outs[0]['actions']), 'action_t1': np.array(outs[1]['actions'])}
    messages = []
    for i, msg in enumerate(queue.messages):
        kind, path, payload = msg
        if kind == 'txt_file':
            messages.append({'kind': kind, 'path': path, 'content': parse_reference_page(payload)})
        else:
            payload = np.asarray(payload)
            assert payload.dtype == np.uint8
            arrays['msg_%03d' % i] = payload
            messages.append({'kind': kind, 'path': path, 'payload': 'msg_%03d' % i})
    meta = {'numpy': np.__version__, 'matplotlib': matplotlib.__version__, 'seed': SEED, 'H': H, 'W': W, 'T': T, 'M': M,
            'ncam': NCAM, 'ndesig': NDESIG, 'desig': DESIG, 'goal': GOAL, 'policy': POLICY, 'last_itr': last_itr,
            'n_predictor_calls': len(fake.actions_seen), 'messages': messages}

    np.savez_compressed(os.path.join(OUT, 'plan_page.npz'), **arrays)
    with open(os.path.join(OUT, 'plan_page.json'), 'w') as f:
        json.dump(mg.jsonable(meta), f, indent=1, sort_keys=True)
    for fn in ('plan_page.json', 'plan_page.npz'):
        print('  %-20s %8d B' % (fn, os.path.getsize(os.path.join(OUT, fn))))


if __name__ == '__main__':
    main()
