"""Architecture table of the registration network: the flow field of the reference's ``Register_Gtruth_Controller``
(``visual_mpc/policy/cem_controllers/register_gtruth_controller.py:7,21,64-66``: ``setup_gdn(gdnconf, gpu_id)`` builds a
warper ``(current, reference) -> warped, flow, warp_pts``).

The reference takes the network from the ``visual_mpc.registration_network`` package, which is not part of the snapshot.
The network below is THIS PROJECT's table (as ``frame_scorer_arch.py`` is for the learned cost); the engine
(``csrc/vf_registration_net.h``), ``HostRegistrationNet`` and the CPU restatement
(``tests/helpers/oracle_registration_net.py``) all implement this table - parity with the original network is unpinned.
Its widths follow the reference's own ``experiments/sawyer/registration_experiments/gdnconf.py`` (``ch_mult``,
``orig_size``, ``normalization: 'None'``, one model per view).

NHWC, float32, ``m = ch_mult`` in {1, 2, 4}, H and W multiples of 8, 16 <= H, W <= 128:

    in    concat[current frame, reference image] on the channel axis, both in [0, 1]    H   x W   x 6
    d1    3x3 stride 1, zero pad 1, + bias, ReLU, 2x2 max-pool                          H/2 x W/2 x 32m
    d2    same, 32m -> 64m                                                              H/4 x W/4 x 64m
    d3    same, 64m -> 128m                                                             H/8 x W/8 x 128m
    u1    3x3 stride 1, zero pad 1, + bias, ReLU, bilinear x2 up-sampling, 128m -> 64m  H/4 x W/4 x 64m
    u2    same, 64m -> 32m                                                              H/2 x W/2 x 32m
    u3    same, 32m -> 16m                                                              H   x W   x 16m
    flow  5x5 stride 1, zero pad 2, + bias, no activation                               H   x W   x 2 = (dx, dy)

No normalisation layers: a pair's flow depends on that pair alone.  The up-sampling is the four-tap bilinear transposed
convolution of arch 3 (per channel, kernel ``1 - |i - 1.5| / 2``, stride 2, padding 1).  ``(dx, dy)`` maps reference pixel
``(r, c)`` to the point ``(c + dx, r + dy)`` of the current frame - what ``vf_register`` takes.  One weight set per view; the
blob is the table in order, views back to back.
"""
import json
import os
from collections import OrderedDict

import numpy as np

FORMAT = 'vf-registration-net-v1'
CH_MULTS = (1, 2, 4)
MAX_SIZE = 128      # the kernels' limit (csrc/vf_registration_net.h: the staged rows of d1; larger sizes are untested)
# (name, kernel size, input channels / m, output channels / m); d1's six input channels do not scale
LAYERS = (('d1', 3, None, 32), ('d2', 3, 32, 64), ('d3', 3, 64, 128), ('u1', 3, 128, 64), ('u2', 3, 64, 32),
          ('u3', 3, 32, 16), ('flow', 5, 16, None))


class RegistrationNetConfig(object):
    def __init__(self, height=64, width=64, ch_mult=4):
        height, width, ch_mult = int(height), int(width), int(ch_mult)
        if ch_mult not in CH_MULTS:
            raise ValueError('ch_mult must be one of %s, got %r' % (CH_MULTS, ch_mult))
        if height % 8 or width % 8 or height < 16 or width < 16:
            raise ValueError('height and width must be multiples of 8 and at least 16, got %dx%d' % (height, width))
        if height > MAX_SIZE or width > MAX_SIZE:
            raise ValueError('the registration kernels support images up to %dx%d, got %dx%d'
                             % (MAX_SIZE, MAX_SIZE, height, width))
        self.height, self.width, self.ch_mult = height, width, ch_mult

    def as_dict(self):
        return dict(height=self.height, width=self.width, ch_mult=self.ch_mult)

    def layers(self):
        """[(name, k, cin, cout, conv height, conv width)]: the size a layer's convolution runs at."""
        m, H, W = self.ch_mult, self.height, self.width
        sizes = {'d1': 1, 'd2': 2, 'd3': 4, 'u1': 8, 'u2': 4, 'u3': 2, 'flow': 1}
        out = []
        for name, k, cin, cout in LAYERS:
            out.append((name, k, 6 if cin is None else cin * m, 2 if cout is None else cout * m,
                        H // sizes[name], W // sizes[name]))
        return out

    def tensor_shapes(self):
        shapes = OrderedDict()
        for name, k, cin, cout, _, _ in self.layers():
            shapes[name + '/w'] = (k, k, cin, cout)
            shapes[name + '/b'] = (cout,)
        return shapes

    def n_floats(self):
        return sum(int(np.prod(s)) for s in self.tensor_shapes().values())

    def macs_per_pair(self):
        """Algorithmic multiply-accumulates of one (current, reference) pair of one view per layer (every tap counted,
        padding included; pooling and up-sampling are not multiplications by weights and are left out)."""
        return OrderedDict((name, h * w * k * k * cin * cout) for name, k, cin, cout, h, w in self.layers())


class RegistrationNetWeights(object):
    """Named float32 tensors of ONE view in canonical layout + (de)serialisation."""

    def __init__(self, cfg, tensors):
        self.cfg = cfg
        want = cfg.tensor_shapes()
        if list(tensors.keys()) != list(want.keys()):
            raise ValueError('tensor set does not match the registration-net table')
        for name, shape in want.items():
            if tuple(tensors[name].shape) != tuple(shape):
                raise ValueError('%s: shape %s, expected %s' % (name, tuple(tensors[name].shape), shape))
        self.tensors = OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in tensors.items())

    @classmethod
    def random(cls, cfg, seed=0, bias_scale=0.1, gain=1.0):
        """Seeded uniform weights (He limit ``gain * sqrt(6 / fan_in)``), biases ``bias_scale * U(-1, 1)``.  Legacy
        ``RandomState`` stream: the same seed gives the same network everywhere."""
        rs = np.random.RandomState(seed)
        tensors = OrderedDict()
        for name, shape in cfg.tensor_shapes().items():
            if name.endswith('/w'):
                lim = gain * np.sqrt(6.0 / int(np.prod(shape[:-1])))
                tensors[name] = rs.uniform(-lim, lim, shape).astype(np.float32)
            else:
                tensors[name] = (bias_scale * rs.uniform(-1, 1, shape)).astype(np.float32)
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
        """Read a view back; with ``cfg`` given, a file of another size or ``ch_mult`` is refused."""
        with open(os.path.join(model_dir, 'manifest.json')) as f:
            manifest = json.load(f)
        if manifest.get('format') != FORMAT:
            raise ValueError('unknown weight file format %r' % manifest.get('format'))
        file_cfg = RegistrationNetConfig(**manifest['config'])
        if cfg is not None:
            mine, theirs = cfg.as_dict(), file_cfg.as_dict()
            for k in ('height', 'width', 'ch_mult'):
                if mine[k] != theirs[k]:
                    raise ValueError('checkpoint %s=%r does not match requested %r' % (k, theirs[k], mine[k]))
            file_cfg = cfg
        blob = np.fromfile(os.path.join(model_dir, 'weights.bin'), dtype='<f4')
        if blob.size != manifest['n_floats'] or blob.size != file_cfg.n_floats():
            raise ValueError('weights.bin holds %d floats, manifest says %d, the table %d'
                             % (blob.size, manifest['n_floats'], file_cfg.n_floats()))
        tensors = OrderedDict()
        for ent in manifest['tensors']:
            n = int(np.prod(ent['shape']))
            tensors[ent['name']] = blob[ent['offset']:ent['offset'] + n].reshape(ent['shape'])
        return cls(file_cfg, tensors)


def random_registration_weights(cfg, ncam=1, seed=0, bias_scale=0.1):
    """One ``RegistrationNetWeights`` per view with seeds ``seed + view``."""
    return [RegistrationNetWeights.random(cfg, seed + v, bias_scale) for v in range(ncam)]


def save_registration_weights(weights, model_dir):
    """``model_dir/view<v>/`` for every view."""
    for v, w in enumerate(weights):
        w.save(os.path.join(model_dir, 'view%d' % v))


def load_registration_weights(model_dir, cfg, ncam=1):
    return [RegistrationNetWeights.load(os.path.join(model_dir, 'view%d' % v), cfg) for v in range(ncam)]


def config_from_gdnconf(conf):
    """The reference's ``gdnconf`` dict (``experiments/sawyer/registration_experiments/gdnconf.py``) ->
    ``(RegistrationNetConfig, [one weight directory per view])``: ``orig_size`` = [height, width], ``ch_mult`` carries
    over, ``pretrained_model`` lists one entry per view.  The table has no normalisation layers, so a ``normalization``
    other than ``'None'`` is refused."""
    norm = conf.get('normalization', 'None')
    if norm not in ('None', None):
        raise ValueError("the registration network has no normalisation layers: normalization=%r is not supported" % (norm,))
    size = conf.get('orig_size', [64, 64])
    paths = conf.get('pretrained_model', [])
    if isinstance(paths, str):
        paths = [paths]
    return RegistrationNetConfig(height=size[0], width=size[1], ch_mult=conf.get('ch_mult', 1)), list(paths)
