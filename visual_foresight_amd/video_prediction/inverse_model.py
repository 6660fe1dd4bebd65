"""The action-inference network of the inverse-model policy behind one Python object.

``HipActionInference`` owns a ``vf_invmodel`` of ``libvf_hip.so`` (``include/vf_hip.h``, "Inverse-model policy"): the table
of ``inverse_model_arch.py`` as HIP kernels that turn (start image, goal image, context actions, context frames) into the
next ``n_actions`` actions without leaving the device.  It has the duck-type of the predictor the reference's
``InvModelBaseController`` builds (``inverse_model_base_controller.py:31-32,79-80``):
``predictor_class(model_params_path, hparams, n_gpus, first_gpu)``, ``restore()``,
``predictor(start, goal, context_actions, context_frames) -> [1, n_actions, adim]``.  ``HostActionInference`` is the same
table on the CPU (PyTorch float32) with the same interface: the controller's CPU path and the timing baseline - never a
substitute for a missing kernel.

hparams (used when ``model_params_path`` is empty; a directory written by ``InverseModelWeights.save`` carries its own):
``image_height``, ``image_width``, ``adim``, ``n_context``, ``n_actions``, ``input_scale``; ``seed`` / ``bias_scale`` / ``gain`` of
the random weights; ``max_batch`` (most problems of one ``infer``, default 1).
"""
import ctypes

import numpy as np

from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction import resample
from visual_foresight_amd.video_prediction.inverse_model_arch import UNITS, InverseModelConfig, InverseModelWeights

MAX_HOST_THREADS = 16


def invmodel_config(hparams):
    hp = dict(hparams)
    return InverseModelConfig(height=hp.get('image_height', 64), width=hp.get('image_width', 64), adim=hp.get('adim', 4),
                              n_context=hp.get('n_context', 2), n_actions=hp.get('n_actions', 15),
                              input_scale=hp.get('input_scale', 1.0))


def resolve_weights(path_or_weights, hparams):
    """An ``InverseModelWeights``, a directory written by its ``save()`` (the manifest supplies the config), or '' / None for
    seeded random weights of the size ``hparams`` names."""
    if isinstance(path_or_weights, InverseModelWeights):
        return path_or_weights
    if path_or_weights:
        return InverseModelWeights.load(path_or_weights)
    hp = dict(hparams)
    return InverseModelWeights.random(invmodel_config(hp), seed=int(hp.get('seed', 0)),
                                      bias_scale=float(hp.get('bias_scale', 0.1)), gain=float(hp.get('gain', 1.0)))


class _ActionInference(object):
    """What both networks share: the predictor call of ``InvModelBaseController`` and the shape checks."""

    def _init_common(self, model_params_path, hparams, n_gpus, first_gpu):
        self._hp = dict(hparams)
        self._source = model_params_path
        self.n_gpus, self.first_gpu = int(n_gpus), int(first_gpu)
        self.max_batch = int(self._hp.get('max_batch', 1))
        self.weights, self.cfg = None, None
        # 'camera_height' / 'camera_width': images arrive at the camera's resolution and are shrunk to the network's
        # (resample.py) before every inference; None (default) = the network's size, and any other size is refused
        cam = (self._hp.get('camera_height'), self._hp.get('camera_width'))
        if (cam[0] is None) != (cam[1] is None):
            raise ValueError("'camera_height' and 'camera_width' come as a pair, got %r x %r" % cam)
        self.camera_size = None if cam[0] is None else (int(cam[0]), int(cam[1]))

    def _at_camera_size(self, start, goal, ctx_frames):
        """True when all three image inputs are at the camera's size (they are then shrunk); at the network's size they go
        in as they are, and ``_check`` refuses everything else."""
        c = self.cfg
        if c is None or self.camera_size is None or self.camera_size == (c.height, c.width):
            return False
        resample.check_aspect(self.camera_size, (c.height, c.width))
        return all(tuple(x.shape[-3:-1]) == self.camera_size for x in (start, goal, ctx_frames))

    def _check(self, start, goal, ctx_actions, ctx_frames):
        c = self.cfg
        if c is None:
            raise ValueError('%s: restore() has not been called' % type(self).__name__)
        n = start.shape[0]
        img = (c.height, c.width, 3)
        for name, arr, want in (('start', start, (n,) + img), ('goal', goal, (n,) + img),
                                ('context_frames', ctx_frames, (n, c.n_context) + img),
                                ('context_actions', ctx_actions, (n, c.n_context, c.adim))):
            if tuple(arr.shape) != want:
                raise ValueError('%s has shape %s; the model wants %s (images of %dx%d, %d context steps, adim %d; images are '
                                 'not resized)' % (name, tuple(arr.shape), want, c.height, c.width, c.n_context, c.adim))

    def __call__(self, start_image, goal_image, context_actions, context_frames):
        """The reference's call: ``start``, ``goal [H, W, 3]``, ``context_actions [1, n_context, adim]``, ``context_frames [1,
        n_context, H, W, 3]`` -> float32 ``[1, n_actions, adim]``."""
        start, goal = np.asarray(start_image), np.asarray(goal_image)
        if start.ndim != 3 or goal.ndim != 3:
            c = self.cfg
            raise ValueError('start and goal image must be [H, W, 3], got %s and %s%s'
                             % (start.shape, goal.shape, '' if c is None else ' (the model wants %dx%d)' % (c.height, c.width)))
        return self.infer(start[None], goal[None], context_actions, context_frames)


class HipActionInference(_ActionInference):
    """``HipActionInference(model_params_path, hparams, n_gpus=1, first_gpu=0)``.  ``n_gpus > 1`` is accepted (the
    reference's constructor signature); the network runs on ``first_gpu``."""

    def __init__(self, model_params_path, hparams, n_gpus=1, first_gpu=0):
        import torch
        self._torch = torch
        self._init_common(model_params_path, hparams, n_gpus, first_gpu)
        if not torch.cuda.is_available():
            raise _lib.VfError('HipActionInference needs a ROCm GPU (no CPU fallback)')
        self.device = torch.device('cuda', self.first_gpu)
        self._libh = _lib.load_library()
        self._handle = ctypes.c_void_p()
        self._c_cfg = None

    def _destroy(self):
        if getattr(self, '_handle', None) and self._handle.value:
            self._libh.vf_invmodel_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self._destroy()
        except Exception:   # interpreter shutdown
            pass

    def restore(self, weights=None):
        torch = self._torch
        self.weights = resolve_weights(weights if weights is not None else self._source, self._hp)
        c = self.cfg = self.weights.cfg
        self._destroy()
        self._c_cfg = _lib.VfInvModelConfig(c.height, c.width, c.adim, c.n_context, c.n_actions, self.max_batch,
                                            self.device.index, c.input_scale)
        blob = self.weights.blob()
        want = self._libh.vf_invmodel_weight_count(ctypes.byref(self._c_cfg))
        if blob.size != want:
            raise _lib.VfError('inverse-model weight blob has %d floats, library expects %d (%s)'
                               % (blob.size, want, self._libh.vf_last_error().decode()))
        with torch.cuda.device(self.device):
            _lib.check(self._libh.vf_invmodel_create(ctypes.byref(self._c_cfg), ctypes.byref(self._handle)))
            _lib.check(self._libh.vf_invmodel_load_weights(self._handle, blob.ctypes.data_as(ctypes.c_void_p), blob.size))
        return self

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _tensor(self, x):
        torch = self._torch
        t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32) if not torch.is_tensor(x) else x)
        return t.to(self.device, torch.float32).contiguous()

    def infer_device(self, start, goal, ctx_actions, ctx_frames, want_hidden=False):
        """``start``, ``goal [n, H, W, 3]``, ``ctx_actions [n, n_context, adim]``, ``ctx_frames [n, n_context, H, W, 3]`` (host or
        device) -> device ``[n, n_actions, adim]`` (and ``[n, n_context + n_actions, 2, 128]`` = h, c after every step)."""
        torch = self._torch
        start, goal, ctx_actions, ctx_frames = (self._tensor(x) for x in (start, goal, ctx_actions, ctx_frames))
        if self._at_camera_size(start, goal, ctx_frames) and start.dim() == 4 and goal.shape == start.shape and \
                ctx_frames.dim() == 5 and ctx_frames.shape[0] == start.shape[0]:
            # camera-size images: one vf_resize_area call (float32 path) for the start images, the goals and the context
            c, n = self.cfg, int(start.shape[0])
            with torch.cuda.device(self.device):
                small = resample.area_resize_device(
                    torch.cat([start, goal, ctx_frames.reshape((-1,) + tuple(ctx_frames.shape[2:]))]), (c.height, c.width))
            start, goal = small[:n], small[n:2 * n]
            ctx_frames = small[2 * n:].reshape((n, -1) + tuple(small.shape[1:]))
        self._check(start, goal, ctx_actions, ctx_frames)
        c, n = self.cfg, int(start.shape[0])
        out = torch.empty((n, c.n_actions, c.adim), dtype=torch.float32, device=self.device)
        hidden = torch.empty((n, c.n_context + c.n_actions, 2, UNITS), dtype=torch.float32, device=self.device) \
            if want_hidden else None
        with torch.cuda.device(self.device):
            _lib.check(self._libh.vf_invmodel_infer(self._handle, start.data_ptr(), goal.data_ptr(), ctx_frames.data_ptr(),
                                                    ctx_actions.data_ptr(), n, out.data_ptr(),
                                                    hidden.data_ptr() if want_hidden else None, self._stream()))
        return (out, hidden) if want_hidden else out

    def infer(self, start, goal, ctx_actions, ctx_frames):
        return self.infer_device(start, goal, ctx_actions, ctx_frames).cpu().numpy()


class HostActionInference(_ActionInference):
    """The table of ``inverse_model_arch.py`` on the CPU in float32 (PyTorch, at most 16 threads).  Same constructor,
    ``restore``, call and ``infer`` as ``HipActionInference``."""

    def __init__(self, model_params_path, hparams, n_gpus=1, first_gpu=0):
        self._init_common(model_params_path, hparams, n_gpus, first_gpu)
        self._params = None

    def restore(self, weights=None):
        import torch
        torch.set_num_threads(min(MAX_HOST_THREADS, torch.get_num_threads()))
        self.weights = resolve_weights(weights if weights is not None else self._source, self._hp)
        self.cfg = self.weights.cfg
        p = {}
        for k, v in self.weights.tensors.items():
            t = torch.from_numpy(v)
            p[k] = t.permute(3, 2, 0, 1).contiguous() if t.dim() == 4 else t       # conv weights as OIHW
        self._params = p
        return self

    def _tower(self, x, name):
        import torch.nn.functional as F
        p = self._params
        x = x.permute(0, 3, 1, 2)
        for l in range(1, 5):
            x = F.relu(F.conv2d(x, p['%s/c%d/w' % (name, l)], p['%s/c%d/b' % (name, l)], stride=2, padding=1))
        return x.flatten(2).mean(dim=2)

    def _cell(self, x, a, h, c):
        import torch
        p = self._params
        z = p['lstm/b'] + x @ p['lstm/wx'] + a @ p['lstm/wa'] + h @ p['lstm/wh']
        i, f, g, o = (z[:, k * UNITS:(k + 1) * UNITS] for k in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    def infer(self, start, goal, ctx_actions, ctx_frames, want_hidden=False):
        import torch
        start, goal, ctx_actions, ctx_frames = (np.ascontiguousarray(x, dtype=np.float32)
                                                for x in (start, goal, ctx_actions, ctx_frames))
        if self._at_camera_size(start, goal, ctx_frames):
            size = (self.cfg.height, self.cfg.width)
            start, goal, ctx_frames = (resample.area_resize_host(x, size) for x in (start, goal, ctx_frames))
        start, goal, ctx_actions, ctx_frames = (torch.from_numpy(x) for x in (start, goal, ctx_actions, ctx_frames))
        self._check(start, goal, ctx_actions, ctx_frames)
        cfg, p, n = self.cfg, self._params, start.shape[0]
        scale = np.float32(cfg.input_scale)
        with torch.no_grad():
            pair = self._tower(torch.cat([goal, start], dim=-1) * scale, 'pair')
            q = self._tower(ctx_frames.reshape((n * cfg.n_context,) + tuple(ctx_frames.shape[2:])) * scale, 'ctx')
            q = q.reshape(n, cfg.n_context, UNITS)
            h = torch.zeros((n, UNITS))
            c = torch.zeros((n, UNITS))
            hidden, actions = [], []
            for i in range(cfg.n_context):
                h, c = self._cell(q[:, i], ctx_actions[:, i], h, c)
                hidden.append(torch.stack([h, c], dim=1))
            a = ctx_actions[:, -1]
            for _ in range(cfg.n_actions):
                h, c = self._cell(pair, a, h, c)
                hidden.append(torch.stack([h, c], dim=1))
                a = p['out/b'] + h @ p['out/w']
                actions.append(a)
            out = torch.stack(actions, dim=1).numpy()
            return (out, torch.stack(hidden, dim=1).numpy()) if want_hidden else out
