"""The plan page of a verbose CEM iteration: what the controllers send to the agent's file worker.

The reference's controllers render the ten best plans after the last CEM iteration and ``put`` them on the agent's file
queue as ``(kind, path, payload)`` tuples (``visual_mpc/policy/cem_controllers/pixel_cost_controller.py:88-131``,
``goal_im_controller.py:101-141``, ``visualizer/construct_html.py:77-93``; consumed by
``visual_mpc/agent/utils/file_saver.py:23-53``).  ``build_plan_messages`` produces that stream from rendered bytes, in
the reference's order and under the reference's names:

    ('img', 'planning_{t}_itr_{i}/assets/cam_{c}_start.jpg', uint8 [H, W, 3])            one per view
    ('img', '.../assets/cam_{c}_goal.jpg', uint8 [H, W, 3])                              goal-image planning only
    ('mov', '.../assets/cam_{c}_desig_{p}_{k}.gif', uint8 [T, H, W, 3])                  view-major, pixel, then plan k
    ('mov', '.../assets/cam_{c}_pred_images_{k}.gif', uint8 [T, H, W, 3])                view-major, then plan k
    ('txt_file', 'planning_{t}_itr_{i}/plan.html', page text)

The page is a table with one column per plan (``traj_0`` ...) and the rows ``cam_{c}_start``, (``cam_{c}_goal``,)
``cam_{c}_desig_{p}``, ``cam_{c}_pred_images``, ``scores``; image cells point to ``assets/...`` relative to the page.  The
markup is this project's own; ``parse_plan_page`` reads its content back (heading, iteration, t, image height, columns,
ordered rows), which is what the tests compare with the reference's page.

A worker that writes other formats announces them as ``asset_extensions = (movie, image)``; without the attribute the
reference's ``('gif', 'jpg')`` are used, so a reference file worker keeps getting the reference's paths.

Not pinned by the reference: the markers of designated (red) and goal (blue) pixels on the start image.  The reference
draws ``cv2.circle(img, (w, h), 1, colour, -1)``; OpenCV is not part of this stack, and here a marker is DEFINED as the
pixel and its four edge neighbours, each drawn only where it lies inside the image; per designated pixel the red marker
first, then the blue one.
"""
from html import escape
from html.parser import HTMLParser

import numpy as np

REFERENCE_EXTENSIONS = ('gif', 'jpg')
DESIG_COLOUR, GOAL_COLOUR = (255, 0, 0), (0, 0, 255)
N_PLANS = 10        # the reference shows scores.argsort()[:10]


def asset_extensions(worker):
    """(movie extension, image extension) of the files ``worker`` writes."""
    return tuple(getattr(worker, 'asset_extensions', REFERENCE_EXTENSIONS))


def draw_marker(img, row, col, colour):
    """The marker defined in the module docstring, drawn into uint8 ``img [H, W, 3]`` in place."""
    r0, c0 = int(row), int(col)
    for dr, dc in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        r, c = r0 + dr, c0 + dc
        if 0 <= r < img.shape[0] and 0 <= c < img.shape[1]:
            img[r, c] = colour
    return img


def mark_start_image(image, desig_pix, goal_pix):
    """A copy of ``image [H, W, 3]`` with the markers of ``desig_pix`` / ``goal_pix [ndesig, 2]`` (row, col)."""
    img = np.array(image, dtype=np.uint8, copy=True)
    for d, g in zip(np.asarray(desig_pix).reshape(-1, 2), np.asarray(goal_pix).reshape(-1, 2)):
        draw_marker(img, d[0], d[1], DESIG_COLOUR)
        draw_marker(img, g[0], g[1], GOAL_COLOUR)
    return img


# ---------------------------------------------------------------------------------------------- the page
_STYLE = """
  body { font-family: sans-serif; margin: 1.5em; }
  table.plans { border-collapse: collapse; }
  table.plans th, table.plans td { border: 1px solid #444; padding: 4px 6px; text-align: center; }
  table.plans th[scope=row] { text-align: left; }
"""


def render_plan_page(cem_itr, t, rows, img_height=128, heading='Visual MPC', column_title='traj'):
    """``rows``: ordered ``(name, cells)`` pairs of equal length; cells that are asset paths become images."""
    rows = [(name, list(cells)) for name, cells in rows]
    widths = {len(cells) for _, cells in rows}
    if len(widths) != 1:
        raise ValueError('every row of a plan page needs the same number of cells, got %s' % sorted(widths))
    n = widths.pop()
    out = ['<!DOCTYPE html>', '<html lang="en">', '<head>', '<meta charset="utf-8">',
           '<title>%s: iteration %s, t = %s</title>' % (escape(str(heading)), cem_itr, t),
           '<style>%s</style>' % _STYLE, '</head>', '<body>',
           '<h1>%s</h1>' % escape(str(heading)),
           '<p>CEM iteration <span id="iteration">%s</span> at time step <span id="t">%s</span></p>' % (cem_itr, t),
           '<table class="plans">', '<thead><tr><th></th>%s</tr></thead>'
           % ''.join('<th scope="col">%s_%d</th>' % (escape(column_title), i) for i in range(n)), '<tbody>']
    for name, cells in rows:
        is_image = isinstance(cells[0], str) and any(ext in cells[0] for ext in ('gif', 'png', 'jpg'))
        tds = []
        for i, cell in enumerate(cells):
            if is_image:
                tds.append('<td><img src="%s" height="%d" alt="%s, plan %d"></td>'
                           % (escape(cell, quote=True), img_height, escape(name, quote=True), i))
            else:
                tds.append('<td>%s</td>' % escape('{}'.format(cell)))
        out.append('<tr><th scope="row">%s</th>%s</tr>' % (escape(name), ''.join(tds)))
    out += ['</tbody>', '</table>', '</body>', '</html>']
    return '\n'.join(out)


class _PageReader(HTMLParser):
    def __init__(self):
        HTMLParser.__init__(self)
        self.content = {'heading': None, 'iteration': None, 't': None, 'image_height': None, 'columns': [], 'rows': []}
        self._field = None      # where the text of the open element goes

    def handle_starttag(self, tag, attrs):
        a = dict(attrs)
        if tag == 'h1':
            self._field = 'heading'
        elif tag == 'span' and a.get('id') in ('iteration', 't'):
            self._field = a['id']
        elif tag == 'th' and a.get('scope') == 'col':
            self._field = 'column'
        elif tag == 'th' and a.get('scope') == 'row':
            self._field = 'row'
        elif tag == 'td':
            self._field = 'cell'
        elif tag == 'img' and self._field == 'cell':
            self.content['rows'][-1][1].append(a['src'])
            heights = {self.content['image_height'], int(a['height'])} - {None}
            if len(heights) != 1:
                raise ValueError('images of differing heights on one plan page')
            self.content['image_height'] = heights.pop()
            self._field = None

    def handle_endtag(self, tag):
        if tag in ('h1', 'span', 'th', 'td'):
            self._field = None

    def handle_data(self, data):
        text, c = data.strip(), self.content
        if not text or self._field is None:
            return
        if self._field in ('heading', 'iteration', 't'):
            c[self._field] = text
        elif self._field == 'column':
            c['columns'].append(text)
        elif self._field == 'row':
            c['rows'].append([text, []])
        elif self._field == 'cell':
            c['rows'][-1][1].append(text)


def parse_plan_page(text):
    """The content of a page of ``render_plan_page``: ``{'heading', 'iteration', 't', 'image_height', 'columns',
    'rows': [[name, [cell, ...]], ...]}`` - numbers as the text the page shows."""
    reader = _PageReader()
    reader.feed(text)
    reader.close()
    return reader.content


# ---------------------------------------------------------------------------------------------- the message stream
def build_plan_messages(t, cem_itr, start_images, scores, frames=None, distributions=None, desig_pix=None,
                        goal_pix=None, goal_images=None, img_height=128, extensions=REFERENCE_EXTENSIONS):
    """-> the ordered ``[(kind, path, payload), ...]`` of one plan page.

    :param start_images: uint8 ``[ncam, H, W, 3]``, the newest observed frame of every view
    :param scores: the K shown plans' scores, best first
    :param frames: uint8 ``[K, ncam, T, H, W, 3]`` rendered predicted frames (``render_plans`` layout)
    :param distributions: uint8 ``[K, ncam, ndesig, T, H, W, 3]`` rendered distributions, or None (no such rows)
    :param desig_pix, goal_pix: ``[ncam, ndesig, 2]`` (row, col) marked on the start images, or None (no markers)
    :param goal_images: uint8 ``[ncam, H, W, 3]`` for the ``cam_{c}_goal`` rows of goal-image planning, or None
    :param extensions: (movie, image) file extensions, see ``asset_extensions``
    """
    mov_ext, img_ext = extensions
    scores = np.asarray(scores)
    K = scores.shape[0]
    start_images = np.asarray(start_images)
    ncam = start_images.shape[0]
    folder = 'planning_{}_itr_{}'.format(t, cem_itr)
    messages, rows = [], []

    def image_row(name, img):
        rel = 'assets/{}.{}'.format(name, img_ext)
        messages.append(('img', '{}/{}'.format(folder, rel), img))
        rows.append((name, [rel] * K))

    def movie_row(name, movies):
        rels = []
        for k, mov in enumerate(movies):
            rels.append('assets/{}_{}.{}'.format(name, k, mov_ext))
            messages.append(('mov', '{}/{}'.format(folder, rels[-1]), np.ascontiguousarray(mov)))
        rows.append((name, rels))

    for c in range(ncam):
        if desig_pix is not None:
            img = mark_start_image(start_images[c], np.asarray(desig_pix)[c], np.asarray(goal_pix)[c])
        else:
            img = np.array(start_images[c], dtype=np.uint8, copy=True)
        image_row('cam_{}_start'.format(c), img)
    if goal_images is not None:
        for c in range(ncam):
            image_row('cam_{}_goal'.format(c), np.asarray(goal_images)[c])
    if distributions is not None:
        if distributions.shape[:2] != (K, ncam):
            raise ValueError('distributions %s do not match %d plans of %d views' % (distributions.shape, K, ncam))
        for c in range(ncam):
            for p in range(distributions.shape[2]):
                movie_row('cam_{}_desig_{}'.format(c, p), distributions[:, c, p])
    if frames is not None:
        if frames.shape[:2] != (K, ncam):
            raise ValueError('frames %s do not match %d plans of %d views' % (frames.shape, K, ncam))
        for c in range(ncam):
            movie_row('cam_{}_pred_images'.format(c), frames[:, c])
    rows.append(('scores', list(scores)))
    page = render_plan_page(cem_itr, t, rows, img_height=img_height)
    messages.append(('txt_file', '{}/plan.html'.format(folder), page))
    return messages


def render_for_page(predictor, indices, context, actions, want_distributions=True):
    """The shown plans' bytes: on the device when ``predictor`` has ``render_plans`` (they are rendered where the last
    scoring call left them), otherwise on the host from what ``predictor(context, ...)`` returns for those actions."""
    from .colormap import render_prediction
    if hasattr(predictor, 'render_plans'):
        return predictor.render_plans(indices, frames=True, distributions=want_distributions)
    prediction = predictor(context, {'actions': np.asarray(actions)[indices]})
    return render_prediction(prediction['predicted_frames'],
                             prediction['predicted_pixel_distributions'] if want_distributions else None)
