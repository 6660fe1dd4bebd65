"""Architecture table of the action-inference network behind the reference's inverse-model policy
(``visual_mpc/policy/inverse_models/inverse_model_base_controller.py:4,31-32,76-80``: ``predictor_class(model_params_path,
{}, n_gpus, first_gpu)``, ``restore()``, then ``predictor(start image, goal image, context actions, context frames) ->
actions [1, T, adim]``).

The reference takes the network from ``robonet.inverse_model.testing.action_inference_interface``, which is not part of
the snapshot.  The network below is THIS PROJECT's table (as ``frame_scorer_arch.py`` and ``registration_net_arch.py`` are
for their networks); the engine (``csrc/vf_inverse_model.h``), ``HostActionInference`` and the CPU restatement
(``tests/helpers/oracle_inverse_model.py``) all implement this table - parity with the original network is unpinned.  Its
interface follows the controller's call (camera 0 only: ``images[-1, 0]``, ``goal_image[-1, 0]``) and the hyper-parameters
of the reference's ``experiments/robonet/inverse_model/*.py`` (``T``, ``num_context``).

NHWC, float32, one weight set; H and W multiples of 16, W <= 128 (the frame scorer's limits):

    pair tower   concat[goal, start] * input_scale (6 channels) through the frame scorer's convolution table
                 (``frame_scorer_arch.CHANNELS``: four 3x3 / 2, zero padding 1, + bias, ReLU, 32-64-128-128), then the mean
                 over the positions in row-major order                                                    -> p   [128]
    ctx tower    the same table with 3 input channels on each of the n_context context frames            -> q_i [128]
    LSTM cell    128 units, gate order i, f, g, o:  z = b + x Wx + a Wa + h Wh   (x in R^128, a in R^adim)
                 c' = sigmoid(f) c + sigmoid(i) tanh(g),  h' = sigmoid(o) tanh(c')
    schedule     h = c = 0;  warm-up  i = 0 .. n_context - 1:  (h, c) = cell(x = q_i, a = context action i)
                 decode   t = 0 .. n_actions - 1:   (h, c) = cell(x = p, a = a_{t-1}),  a_t = bo + h Wo,
                 a_{-1} = the last context action

The blob is the table in order: ``pair/c1..c4/{w,b}``, ``ctx/c1..c4/{w,b}``, ``lstm/wx [128][512]``, ``lstm/wa [adim][512]``,
``lstm/wh [128][512]``, ``lstm/b [512]``, ``out/w [128][adim]``, ``out/b [adim]``.
"""
import json
import os
from collections import OrderedDict

import numpy as np

from visual_foresight_amd.video_prediction.frame_scorer_arch import CHANNELS

FORMAT = 'vf-inverse-model-v1'
UNITS = 128             # LSTM width = CHANNELS[-1]
MAX_WIDTH = 128         # the kernels' limit (csrc/vf_inverse_model.h: the staged rows of c1)
TOWERS = (('pair', 6), ('ctx', 3))


class InverseModelConfig(object):
    def __init__(self, height=64, width=64, adim=4, n_context=2, n_actions=15, input_scale=1.0):
        height, width, adim, n_context, n_actions = int(height), int(width), int(adim), int(n_context), int(n_actions)
        if height % 16 or width % 16 or height < 16 or width < 16:
            raise ValueError('height and width must be multiples of 16, got %dx%d' % (height, width))
        if width > MAX_WIDTH:
            raise ValueError('width must be at most %d, got %d' % (MAX_WIDTH, width))
        if not 1 <= adim <= 8:
            raise ValueError('adim must be 1..8, got %d' % adim)
        if not 1 <= n_context <= 4:
            raise ValueError('n_context must be 1..4, got %d' % n_context)
        if not 1 <= n_actions <= 32:
            raise ValueError('n_actions must be 1..32, got %d' % n_actions)
        if not float(input_scale) > 0:
            raise ValueError('input_scale must be positive, got %r' % (input_scale,))
        self.height, self.width, self.adim = height, width, adim
        self.n_context, self.n_actions, self.input_scale = n_context, n_actions, float(input_scale)

    def as_dict(self):
        return dict(height=self.height, width=self.width, adim=self.adim, n_context=self.n_context,
                    n_actions=self.n_actions, input_scale=self.input_scale)

    def tensor_shapes(self):
        shapes = OrderedDict()
        for tower, cin in TOWERS:
            for i, cout in enumerate(CHANNELS):
                shapes['%s/c%d/w' % (tower, i + 1)] = (3, 3, cin, cout)
                shapes['%s/c%d/b' % (tower, i + 1)] = (cout,)
                cin = cout
        shapes['lstm/wx'] = (UNITS, 4 * UNITS)
        shapes['lstm/wa'] = (self.adim, 4 * UNITS)
        shapes['lstm/wh'] = (UNITS, 4 * UNITS)
        shapes['lstm/b'] = (4 * UNITS,)
        shapes['out/w'] = (UNITS, self.adim)
        shapes['out/b'] = (self.adim,)
        return shapes

    def n_floats(self):
        return sum(int(np.prod(s)) for s in self.tensor_shapes().values())


class InverseModelWeights(object):
    """Named float32 tensors in canonical layout + (de)serialisation."""

    def __init__(self, cfg, tensors):
        self.cfg = cfg
        want = cfg.tensor_shapes()
        if list(tensors.keys()) != list(want.keys()):
            raise ValueError('tensor set does not match the inverse-model table')
        for name, shape in want.items():
            if tuple(tensors[name].shape) != tuple(shape):
                raise ValueError('%s: shape %s, expected %s' % (name, tuple(tensors[name].shape), shape))
        self.tensors = OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in tensors.items())

    @classmethod
    def random(cls, cfg, seed=0, bias_scale=0.1, gain=1.0):
        """Seeded uniform weights, biases ``bias_scale * U(-1, 1)``.  Convolutions: the He limit ``gain * sqrt(6 / fan_in)``
        (activations keep their size through the ReLUs).  ``lstm/wx``, ``lstm/wh``, ``out/w``: ``gain * sqrt(3 / 128)`` and
        ``lstm/wa``: ``gain * sqrt(3 / adim)`` - each term of a gate sum has about the variance of its input, so with pooled
        features and actions of order one the gates stay in the sloped part of the sigmoid (chosen on the CPU: the float32
        restatement gives actions that vary over ``t`` and move with the goal).  Legacy ``RandomState`` stream: the same
        seed gives the same network everywhere."""
        rs = np.random.RandomState(seed)
        tensors = OrderedDict()
        for name, shape in cfg.tensor_shapes().items():
            if name.endswith('/b'):
                tensors[name] = (bias_scale * rs.uniform(-1, 1, shape)).astype(np.float32)
                continue
            fan_in = int(np.prod(shape[:-1]))
            lim = gain * np.sqrt((6.0 if '/c' in name else 3.0) / fan_in)
            tensors[name] = rs.uniform(-lim, lim, shape).astype(np.float32)
        return cls(cfg, tensors)

    def blob(self):
        return np.concatenate([v.ravel() for v in self.tensors.values()]).astype(np.float32)

    def n_floats(self):
        return sum(v.size for v in self.tensors.values())

    def save(self, model_dir):
        """``model_dir/manifest.json`` + ``model_dir/weights.bin`` (flat little-endian float32)."""
        os.makedirs(model_dir, exist_ok=True)
        manifest = {'format': FORMAT, 'config': self.cfg.as_dict(), 'tensors': []}
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
    def load(cls, model_dir, cfg=None):
        """Read a model back; with ``cfg`` given, a file of another size, ``adim``, ``n_context`` or ``n_actions`` is
        refused (``input_scale`` is the file's)."""
        with open(os.path.join(model_dir, 'manifest.json')) as f:
            manifest = json.load(f)
        if manifest.get('format') != FORMAT:
            raise ValueError('unknown weight file format %r' % manifest.get('format'))
        file_cfg = InverseModelConfig(**manifest['config'])
        if cfg is not None:
            mine, theirs = cfg.as_dict(), file_cfg.as_dict()
            for k in ('height', 'width', 'adim', 'n_context', 'n_actions'):
                if mine[k] != theirs[k]:
                    raise ValueError('checkpoint %s=%r does not match requested %r' % (k, theirs[k], mine[k]))
        blob = np.fromfile(os.path.join(model_dir, 'weights.bin'), dtype='<f4')
        if blob.size != manifest['n_floats'] or blob.size != file_cfg.n_floats():
            raise ValueError('weights.bin holds %d floats, manifest says %d, the table %d'
                             % (blob.size, manifest['n_floats'], file_cfg.n_floats()))
        tensors = OrderedDict()
        for ent in manifest['tensors']:
            n = int(np.prod(ent['shape']))
            tensors[ent['name']] = blob[ent['offset']:ent['offset'] + n].reshape(ent['shape'])
        return cls(file_cfg, tensors)
