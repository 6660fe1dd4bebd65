"""The frame scorer of learned-cost planning behind one Python object per device.

``HipFrameScorer`` owns a ``vf_scorer`` of ``libvf_hip.so`` (``include/vf_hip.h``, "Learned-cost planning"): the network of
``frame_scorer_arch.py`` as HIP kernels that read the frames a rollout left in the engine.  It replaces the reference's
``control_embedding.deploy_simple_model`` / ``deploy_model`` (``classifier_controller.py:34-36``,
``nce_cost_controller.py:33-35``).  ``HostFrameScorer`` is the same table on the CPU (PyTorch), for predictors whose
frames are on the host anyway - the controllers' fallback, never a substitute for a missing kernel.
"""
import ctypes

import numpy as np

from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.frame_scorer_arch import (FrameScorerConfig, FrameScorerWeights,
                                                                     load_scorer_weights, random_scorer_weights)


def scorer_config(hparams):
    hp = dict(hparams)
    return FrameScorerConfig(height=hp.get('image_height', 64), width=hp.get('image_width', 64),
                             head=hp.get('head', 'classifier'), embed_dim=hp.get('embed_dim', 64),
                             input_scale=hp.get('input_scale'))


def resolve_weights(path_or_weights, cfg, ncam, seed=0, bias_scale=0.1):
    """A directory written by ``save_scorer_weights``, a ``{tower: [per view]}`` dict, or '' / None for seeded random
    weights (as ``model_path=''`` does for the predictor)."""
    if isinstance(path_or_weights, dict):
        weights = path_or_weights
    elif path_or_weights:
        weights = load_scorer_weights(path_or_weights, cfg, ncam)
    else:
        weights = random_scorer_weights(cfg, ncam, seed=seed, bias_scale=bias_scale)
    for tw in cfg.towers:
        views = weights.get(tw)
        if views is None or len(views) != ncam:
            raise ValueError('need %d weight set(s) for the %r tower' % (ncam, tw))
        for w in views:
            if not isinstance(w, FrameScorerWeights) or w.tower != tw or w.cfg.head != cfg.head or \
                    (w.cfg.height, w.cfg.width, w.cfg.out_dim) != (cfg.height, cfg.width, cfg.out_dim):
                raise ValueError('weights of another head, size or tower given for the %r tower' % tw)
    return weights


class HipFrameScorer(object):
    """``HipFrameScorer(path_or_weights, hparams, device)``; hparams: ``image_height``, ``image_width``, ``ncam``, ``head``
    (``'classifier'`` | ``'embedding'``), ``embed_dim``, ``input_scale``, ``max_frames`` (most frames per view of one call:
    the predictor's ``run_batch_size * T``), ``seed`` / ``bias_scale`` of the random weights."""

    def __init__(self, path_or_weights, hparams, device=0):
        import torch
        self._torch = torch
        hp = dict(hparams)
        self._hp = hp
        self.cfg = scorer_config(hp)
        self.n_cam = int(hp.get('ncam', 1))
        self.max_frames = int(hp.get('max_frames', 2600))
        self._source = path_or_weights
        self._seed, self._bias_scale = int(hp.get('seed', 0)), float(hp.get('bias_scale', 0.1))
        if not torch.cuda.is_available():
            raise _lib.VfError('HipFrameScorer needs a ROCm GPU (no CPU fallback)')
        self.device = torch.device('cuda', device.index if isinstance(device, torch.device) else int(device))
        self._libh = _lib.load_library()
        c = self.cfg
        self._c_cfg = _lib.VfScorerConfig(c.height, c.width, self.n_cam, c.head_id, c.embed_dim, self.max_frames,
                                          self.device.index, c.input_scale)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._libh.vf_scorer_create(ctypes.byref(self._c_cfg), ctypes.byref(self._handle)))
        self.weights = None

    def __del__(self):
        try:
            if getattr(self, '_handle', None) and self._handle.value:
                self._libh.vf_scorer_destroy(self._handle)
                self._handle = ctypes.c_void_p()
        except Exception:   # interpreter shutdown
            pass

    def restore(self, weights=None):
        self.weights = resolve_weights(weights if weights is not None else self._source, self.cfg, self.n_cam,
                                       self._seed, self._bias_scale)
        for i, tw in enumerate(self.cfg.towers):
            blob = np.concatenate([w.blob() for w in self.weights[tw]])
            want = self._libh.vf_scorer_weight_count(ctypes.byref(self._c_cfg), i) * self.n_cam
            if blob.size != want:
                raise _lib.VfError('scorer weight blob has %d floats, library expects %d' % (blob.size, want))
            with self._torch.cuda.device(self.device):
                _lib.check(self._libh.vf_scorer_load_weights(self._handle, i, blob.ctypes.data_as(ctypes.c_void_p),
                                                             blob.size))
        return self

    def clone_to(self, device):
        """The same network on another device (one scorer per lane of an in-process multi-GPU predictor)."""
        return HipFrameScorer(self.weights, self._hp, device).restore()

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def embed_device(self, images, tower='frames'):
        """``images [n, ncam, H, W, Cin]`` (host or device, in the scale of predicted frames) -> device ``[n, ncam, D]``."""
        torch, c = self._torch, self.cfg
        t = torch.as_tensor(np.ascontiguousarray(images, dtype=np.float32) if not torch.is_tensor(images) else images)
        t = t.to(self.device, torch.float32).contiguous()
        if tuple(t.shape[1:]) != (self.n_cam, c.height, c.width, c.in_channels(tower)):
            raise ValueError('images must be [n, %d, %d, %d, %d], got %s'
                             % (self.n_cam, c.height, c.width, c.in_channels(tower), tuple(t.shape)))
        out = torch.empty((t.shape[0], self.n_cam, c.out_dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._libh.vf_scorer_embed(self._handle, c.towers.index(tower), t.data_ptr(), int(t.shape[0]),
                                                  out.data_ptr(), self._stream()))
        return out

    def embed(self, images, tower='frames'):
        return self.embed_device(images, tower).cpu().numpy()

    def goal_enc(self, goal_image, start_image):
        """``goal_image`` / ``start_image [ncam, H, W, 3]`` in the scale of predicted frames -> ``goal_enc [ncam, D]``: the
        goal tower on ``concat[goal, start]`` (nce_cost_controller.py:94-98)."""
        pair = np.concatenate([np.asarray(goal_image, np.float32), np.asarray(start_image, np.float32)], axis=-1)
        return self.embed(pair[None], 'goal')[0]


class HostFrameScorer(object):
    """The table of ``frame_scorer_arch.py`` on the CPU in float32 (PyTorch): scores frames that a predictor returned to
    the host.  Same constructor and ``embed`` / ``goal_enc`` as ``HipFrameScorer``."""

    def __init__(self, path_or_weights, hparams, device=None):
        hp = dict(hparams)
        self.cfg = scorer_config(hp)
        self.n_cam = int(hp.get('ncam', 1))
        self._source = path_or_weights
        self._seed, self._bias_scale = int(hp.get('seed', 0)), float(hp.get('bias_scale', 0.1))
        self.weights = None

    def restore(self, weights=None):
        self.weights = resolve_weights(weights if weights is not None else self._source, self.cfg, self.n_cam,
                                       self._seed, self._bias_scale)
        return self

    def _forward(self, w, x):
        import torch
        import torch.nn.functional as F
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) * torch.tensor(self.cfg.input_scale, dtype=torch.float32)
        x = x.permute(0, 3, 1, 2)
        for i in range(1, 5):
            k = torch.from_numpy(w.tensors['c%d/w' % i]).permute(3, 2, 0, 1).contiguous()
            x = F.relu(F.conv2d(x, k, torch.from_numpy(w.tensors['c%d/b' % i]), stride=2, padding=1))
        x = x.mean(dim=(2, 3))
        return (x @ torch.from_numpy(w.tensors['fc/w']) + torch.from_numpy(w.tensors['fc/b'])).numpy()

    def embed(self, images, tower='frames', batch=256):
        images = np.asarray(images)
        n = images.shape[0]
        out = np.empty((n, self.n_cam, self.cfg.out_dim), np.float32)
        for c in range(self.n_cam):
            for i in range(0, n, batch):
                out[i:i + batch, c] = self._forward(self.weights[tower][c], images[i:i + batch, c])
        return out

    def goal_enc(self, goal_image, start_image):
        pair = np.concatenate([np.asarray(goal_image, np.float32), np.asarray(start_image, np.float32)], axis=-1)
        return self.embed(pair[None], 'goal')[0]
