"""Architecture table of the frame scorer: the learned cost of the reference's ``ClassifierController`` and
``NCECostController`` (``visual_mpc/policy/cem_controllers/variants/classifier_controller.py:34-36,94-105``,
``nce_cost_controller.py:33-35,90-103``).

The reference takes its scorer from the ``control_embedding`` package, which is not part of the snapshot.  The network
below is this project's specification (as ``cdna_arch.py`` is for the predictor); the engine (``csrc/vf_frame_scorer.h``)
and the CPU restatement (``tests/helpers/oracle_frame_scorer.py``) both implement THIS table - parity with the original
network is unpinned.

NHWC, float32, frame ``[H][W][Cin]`` with H and W multiples of 16:

    in   frame (in [0, 1]) * input_scale (float32)                        H    x W    x Cin
    c1   3x3 stride 2, zero padding 1 on every side, + bias, ReLU         H/2  x W/2  x 32
    c2   same, 32 -> 64                                                   H/4  x W/4  x 64
    c3   same, 64 -> 128                                                  H/8  x W/8  x 128
    c4   same, 128 -> 128                                                 H/16 x W/16 x 128
    gap  mean over the positions, row-major order                         128
    fc   128 -> D + bias; 'classifier': D = 2 (logits), 'embedding': D = embed_dim

No normalisation layers: a frame's output depends on that frame alone.  The embedding head has a second tower, ``goal``,
with the same table and six input channels - ``concat[goal image, start image]`` - run once per ``act()``
(``scoring_func(goal, start, input_images) -> {'goal_enc', 'input_enc'}``, ``nce_cost_controller.py:94-99``).  One view =
one weight set per tower; the blob is the table concatenated in order, views back to back.
"""
import json
import os
from collections import OrderedDict

import numpy as np

CHANNELS = (32, 64, 128, 128)
HEADS = ('classifier', 'embedding')
TOWERS = ('frames', 'goal')


class FrameScorerConfig(object):
    def __init__(self, height=64, width=64, head='classifier', embed_dim=64, input_scale=None):
        if head not in HEADS:
            raise ValueError("head must be 'classifier' or 'embedding', got %r" % (head,))
        if height % 16 or width % 16 or height < 16 or width < 16:
            raise ValueError('height and width must be multiples of 16, got %dx%d' % (height, width))
        self.height, self.width, self.head = int(height), int(width), head
        self.embed_dim = int(embed_dim)
        # the reference feeds gen_images * 255. / 255 to the classifier and gen_images * 255. to the embedding
        self.input_scale = float(input_scale) if input_scale is not None else (1.0 if head == 'classifier' else 255.0)

    @property
    def out_dim(self):
        return 2 if self.head == 'classifier' else self.embed_dim

    @property
    def head_id(self):
        return HEADS.index(self.head)

    @property
    def towers(self):
        return TOWERS[:1] if self.head == 'classifier' else TOWERS

    def in_channels(self, tower='frames'):
        if tower not in self.towers:
            raise ValueError('the %s head has no %r tower' % (self.head, tower))
        return 3 if tower == 'frames' else 6

    def as_dict(self):
        return dict(height=self.height, width=self.width, head=self.head, embed_dim=self.embed_dim,
                    input_scale=self.input_scale)

    def tensor_shapes(self, tower='frames'):
        shapes = OrderedDict()
        cin = self.in_channels(tower)
        for i, cout in enumerate(CHANNELS):
            shapes['c%d/w' % (i + 1)] = (3, 3, cin, cout)
            shapes['c%d/b' % (i + 1)] = (cout,)
            cin = cout
        shapes['fc/w'] = (CHANNELS[-1], self.out_dim)
        shapes['fc/b'] = (self.out_dim,)
        return shapes

    def macs_per_frame(self, tower='frames'):
        """Algorithmic multiply-accumulates of one frame per layer (the convolutions count every tap, padding included)."""
        out = OrderedDict()
        cin, h, w = self.in_channels(tower), self.height, self.width
        for i, cout in enumerate(CHANNELS):
            h, w = h // 2, w // 2
            out['c%d' % (i + 1)] = h * w * 9 * cin * cout
            cin = cout
        out['fc'] = CHANNELS[-1] * self.out_dim
        return out


class FrameScorerWeights(object):
    """Named float32 tensors of ONE view's tower in canonical layout + (de)serialisation."""

    def __init__(self, cfg, tensors, tower='frames'):
        self.cfg, self.tower = cfg, tower
        want = cfg.tensor_shapes(tower)
        if list(tensors.keys()) != list(want.keys()):
            raise ValueError('tensor set does not match the frame-scorer table')
        for name, shape in want.items():
            if tuple(tensors[name].shape) != tuple(shape):
                raise ValueError('%s: shape %s, expected %s' % (name, tuple(tensors[name].shape), shape))
        self.tensors = OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in tensors.items())

    @classmethod
    def random(cls, cfg, seed=0, bias_scale=0.0, tower='frames', gain=1.0):
        """Seeded uniform weights (He limit ``gain * sqrt(6 / fan_in)``, so activations keep their size through the ReLUs);
        biases ``bias_scale * U(-1, 1)`` - with zero biases and frames that differ little every frame scores alike.  Legacy
        ``RandomState`` stream: the same seed gives the same network everywhere."""
        rs = np.random.RandomState(seed)
        tensors = OrderedDict()
        for name, shape in cfg.tensor_shapes(tower).items():
            if name.endswith('/w'):
                fan_in = int(np.prod(shape[:-1]))
                lim = gain * np.sqrt(6.0 / fan_in)
                tensors[name] = rs.uniform(-lim, lim, shape).astype(np.float32)
            else:
                tensors[name] = (bias_scale * rs.uniform(-1, 1, shape)).astype(np.float32)
        return cls(cfg, tensors, tower)

    def blob(self):
        return np.concatenate([v.ravel() for v in self.tensors.values()]).astype(np.float32)

    def n_floats(self):
        return sum(v.size for v in self.tensors.values())

    def save(self, model_dir):
        """``model_dir/manifest.json`` + ``model_dir/weights.bin`` (flat little-endian float32)."""
        os.makedirs(model_dir, exist_ok=True)
        manifest = {'format': 'vf-frame-scorer-v1', 'tower': self.tower, 'config': self.cfg.as_dict(), 'tensors': []}
        offset = 0
        with open(os.path.join(model_dir, 'weights.bin'), 'wb') as f:
            for name, arr in self.tensors.items():
                manifest['tensors'].append({'name': name, 'shape': list(arr.shape), 'offset': offset})
                f.write(arr.astype('<f4').tobytes())
                offset += arr.size
        manifest['n_floats'] = offset
        with open(os.path.join(model_dir, 'manifest.json'), 'w') as f:
            json.dump(manifest, f, indent=1)

    @classmethod
    def load(cls, model_dir, cfg=None, tower=None):
        """Read a tower back; with ``cfg`` / ``tower`` given, a file of another head, size, embedding width or tower is
        refused."""
        with open(os.path.join(model_dir, 'manifest.json')) as f:
            manifest = json.load(f)
        if manifest.get('format') != 'vf-frame-scorer-v1':
            raise ValueError('unknown weight file format %r' % manifest.get('format'))
        file_cfg = FrameScorerConfig(**manifest['config'])
        file_tower = manifest.get('tower', 'frames')
        if tower is not None and tower != file_tower:
            raise ValueError('checkpoint holds the %r tower, %r was asked for' % (file_tower, tower))
        if cfg is not None:
            mine, theirs = cfg.as_dict(), file_cfg.as_dict()
            for k in ('height', 'width', 'head') + (('embed_dim',) if cfg.head == 'embedding' else ()):
                if mine[k] != theirs[k]:
                    raise ValueError('checkpoint %s=%r does not match requested %r' % (k, theirs[k], mine[k]))
            file_cfg = cfg
        blob = np.fromfile(os.path.join(model_dir, 'weights.bin'), dtype='<f4')
        if blob.size != manifest['n_floats']:
            raise ValueError('weights.bin holds %d floats, manifest says %d' % (blob.size, manifest['n_floats']))
        tensors = OrderedDict()
        for ent in manifest['tensors']:
            n = int(np.prod(ent['shape']))
            tensors[ent['name']] = blob[ent['offset']:ent['offset'] + n].reshape(ent['shape'])
        return cls(file_cfg, tensors, file_tower)


def random_scorer_weights(cfg, ncam=1, seed=0, bias_scale=0.1):
    """``{tower: [one FrameScorerWeights per view]}`` with seeds ``seed + 2 * view (+ 1 for the goal tower)``."""
    return OrderedDict((tw, [FrameScorerWeights.random(cfg, seed + 2 * v + i, bias_scale, tw) for v in range(ncam)])
                       for i, tw in enumerate(cfg.towers))


def save_scorer_weights(weights, model_dir):
    """``model_dir/<tower>/view<v>/`` for every tower and view (what ``*_restore_path`` points at)."""
    for tw, views in weights.items():
        for v, w in enumerate(views):
            w.save(os.path.join(model_dir, tw, 'view%d' % v))


def load_scorer_weights(model_dir, cfg, ncam=1):
    return OrderedDict((tw, [FrameScorerWeights.load(os.path.join(model_dir, tw, 'view%d' % v), cfg, tw)
                             for v in range(ncam)]) for tw in cfg.towers)


# ---------------------------------------------------------------------------------------------- cost arithmetic (host)
LOG_SHIFT = 1e-5        # classifier_controller.py:10


def classifier_raw_cost(logits):
    """``logits [..., ncam, 2]`` (float32 head outputs) -> ``-log(softmax(logits)[1] + 1e-5)`` summed over views, float64
    (classifier_controller.py:102-104)."""
    z = np.asarray(logits, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    e = np.exp(z - m)
    p1 = e[..., 1] / (e[..., 0] + e[..., 1])
    return (-np.log(p1 + LOG_SHIFT)).sum(axis=-1)


def embedding_raw_cost(goal_enc, enc):
    """``goal_enc [ncam, D]``, ``enc [..., ncam, D]`` -> ``-<goal_enc, enc>`` summed over views, float64, d ascending
    (nce_cost_controller.py:100-102,160-164)."""
    g = np.asarray(goal_enc, dtype=np.float64)
    e = np.asarray(enc, dtype=np.float64)
    dot = np.zeros(e.shape[:-1])
    for d in range(e.shape[-1]):
        dot += g[..., d] * e[..., d]
    return (-dot).sum(axis=-1)


def weight_scores(raw, finalweight):
    """``raw [B, T]`` -> ``[B]`` (classifier_controller.py:135-142)."""
    raw = np.asarray(raw, dtype=np.float64)
    T = raw.shape[1]
    if finalweight >= 0:
        acc = np.zeros(raw.shape[0])
        for t in range(T - 1):
            acc += raw[:, t]
        acc += float(finalweight) * raw[:, -1]
        return acc / (float(T - 1) + float(finalweight))
    return raw[:, -1].copy()


def learned_cost(head, head_out, goal_enc=None, finalweight=100., n_draws=1):
    """Head outputs ``[B, T, ncam, D]`` (B = actions * n_draws, draw-minor) -> (scores [A], cost_per_step [A, T]): the
    arithmetic of ``vf_scorer_scores`` on the host, float64."""
    raw = classifier_raw_cost(head_out) if head == 'classifier' else embedding_raw_cost(goal_enc, head_out)
    B, T = raw.shape
    A = B // n_draws
    per_seq = weight_scores(raw, finalweight).reshape(A, n_draws)
    scores = np.zeros(A)
    for j in range(n_draws):
        scores += per_seq[:, j]
    cps = np.zeros((A, T))
    for j in range(n_draws):
        cps += raw.reshape(A, n_draws, T)[:, j]
    return scores / n_draws, cps / n_draws
