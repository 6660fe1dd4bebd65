"""Area resampling: shrinking images from the camera's resolution to the model's.

The reference's agent shrinks every observation with ``cv2.resize(..., INTER_AREA)`` before the policy sees it
(``visual_mpc/utils/im_utils.py:6-15``, ``agent/general_agent.py:128``); ``GoalImController`` shrinks its goal picture the same
way (``goal_im_controller.py:89``) and ``Register_Gtruth_Controller`` its context (``register_gtruth_controller.py:44-51``).

Specification (this project's own; it is meant to be INTER_AREA for shrinking, but ``cv2`` was not available
to pin that - OpenCV's integer-factor fast path may round ties differently).  The exact area average with integer weights per
axis: destination index ``i`` covers ``[i*S, (i+1)*S)`` and source index ``r`` covers ``[r*D, (r+1)*D)`` of one axis of length
``S*D``; ``w[i][r]`` is the length of their overlap, ``sum_r w[i][r] = S``.  With ``A = Hs*Ws``:

* uint8: ``S = sum_r sum_c wy*wx*v`` (an exact integer), output ``S / A`` rounded half to even;
* float32: one float64 sum per output element, source rows ascending and columns ascending within a row, every term
  ``float64(wy*wx) * float64(v)`` (exact), then one float64 division by ``A`` and one rounding to float32.

Equal sizes give a copy: exactly for uint8; for float32 of every value but not of every bit - the sum starts at ``+0.0``, so
``-0.0`` comes back as ``+0.0`` (here and in the kernel alike).

``area_resize_host`` restates that in NumPy (it is what the tests hold the kernel to, bit for bit); ``area_resize_device``
calls ``vf_resize_area`` (``csrc/vf_resize.h``) on a torch tensor.
"""
import ctypes

import numpy as np

from visual_foresight_amd import _lib

MAX_AREA = 1 << 22      # Hs * Ws: the uint8 sum stays below 2^30


def area_weights(S, D):
    """``w[D, S]`` int64: overlap of destination cell ``i`` = ``[i*S, (i+1)*S)`` with source cell ``r`` = ``[r*D, (r+1)*D)``."""
    S, D = int(S), int(D)
    if not 1 <= D <= S:
        raise ValueError('area resampling shrinks only: need 1 <= %d <= %d' % (D, S))
    i = np.arange(D, dtype=np.int64)[:, None]
    r = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((i + 1) * S, (r + 1) * D) - np.maximum(i * S, r * D), 0)


def _check_sizes(shape, size):
    if len(shape) < 3:
        raise ValueError('need an image array [..., H, W, C], got shape %s' % (tuple(shape),))
    Hs, Ws, C = (int(v) for v in shape[-3:])
    Hd, Wd = (int(v) for v in size)
    if not 1 <= C <= 4:
        raise ValueError('C = %d channels outside 1..4' % C)
    if not (1 <= Hd <= Hs and 1 <= Wd <= Ws):
        raise ValueError('area resampling shrinks only: %d x %d -> %d x %d' % (Hs, Ws, Hd, Wd))
    if Hs * Ws > MAX_AREA:
        raise ValueError('Hs*Ws = %d exceeds 2^22' % (Hs * Ws))
    return Hs, Ws, C, Hd, Wd


def _footprints(w):
    """First source index of every destination index and the longest footprint of ``w[D, S]``."""
    first = (w > 0).argmax(axis=1)
    count = (w > 0).sum(axis=1)
    return first, int(count.max())


def area_resize_host(x, size):
    """``x`` uint8 or float32 ``[..., Hs, Ws, C]`` -> ``[..., Hd, Wd, C]`` of the same dtype (``size = (Hd, Wd)``): the
    specification of ``vf_resize_area``, int64 arithmetic for uint8 and a float64 loop in the stated order for float32."""
    x = np.asarray(x)
    Hs, Ws, C, Hd, Wd = _check_sizes(x.shape, size)
    wy, wx = area_weights(Hs, Hd), area_weights(Ws, Wd)
    A = Hs * Ws
    if x.dtype not in (np.uint8, np.float32):
        raise ValueError('area_resize_host takes uint8 or float32, got %s' % x.dtype)
    # one sum per output element over its footprint, vectorised over the outputs: int64 for uint8 (any order gives the
    # same integer), float64 for float32 - there the order of the two loops IS the specification
    wide = np.int64 if x.dtype == np.uint8 else np.float64
    r0, ny = _footprints(wy)
    c0, nx = _footprints(wx)
    v = x.astype(wide)
    rows_i = np.arange(Hd)
    cols_j = np.arange(Wd)
    acc = np.zeros(x.shape[:-3] + (Hd, Wd, C), wide)
    for a in range(ny):                 # source rows of the footprint, ascending
        r = np.minimum(r0 + a, Hs - 1)
        w_r = np.where(r0 + a < Hs, wy[rows_i, r], 0)
        for b in range(nx):             # columns within the row, ascending
            c = np.minimum(c0 + b, Ws - 1)
            w_c = np.where(c0 + b < Ws, wx[cols_j, c], 0)
            w = (w_r[:, None] * w_c[None, :])[:, :, None]
            term = w.astype(wide) * v[..., r[:, None], c[None, :], :]       # (exact in float64: 22 bits times 24)
            acc = np.where(w > 0, acc + term, acc)
    if x.dtype == np.uint8:
        q, rem = acc // A, acc % A
        q = q + ((2 * rem > A) | ((2 * rem == A) & (q % 2 == 1)))
        return q.astype(np.uint8)
    return (acc / np.float64(A)).astype(np.float32)


def area_resize_device(t, size, stream=None):
    """``t``: a contiguous torch uint8 or float32 tensor ``[..., Hs, Ws, C]`` on a GPU -> a new tensor ``[..., Hd, Wd, C]`` on
    the same device (one ``vf_resize_area`` launch on ``stream``, default the current stream of that device)."""
    import torch
    if not t.is_cuda:
        raise ValueError('area_resize_device needs a tensor on a GPU (area_resize_host is the NumPy path)')
    if not t.is_contiguous():
        raise ValueError('area_resize_device needs a contiguous tensor')
    if t.dtype not in (torch.uint8, torch.float32):
        raise ValueError('area_resize_device takes uint8 or float32, got %s' % t.dtype)
    Hs, Ws, C, Hd, Wd = _check_sizes(t.shape, size)
    n = int(np.prod(t.shape[:-3], dtype=np.int64))
    out = torch.empty(tuple(t.shape[:-3]) + (Hd, Wd, C), dtype=t.dtype, device=t.device)
    if n == 0:
        return out
    if stream is None:
        stream = torch.cuda.current_stream(t.device)
    handle = getattr(stream, 'cuda_stream', stream)
    with torch.cuda.device(t.device):       # the library selects the device: put the caller's back
        _lib.check(_lib.load_library().vf_resize_area(
            t.device.index, t.data_ptr(), out.data_ptr(), 0 if t.dtype == torch.uint8 else 1, n, Hs, Ws, C, Hd, Wd,
            ctypes.c_void_p(handle)))
    return out


def check_aspect(camera, model):
    """The reference scales rows and columns by the one ratio ``img_height / image_height``
    (``register_gtruth_controller.py:172``): the two sizes must have one aspect ratio, and the model's may not be larger."""
    (Hc, Wc), (Hm, Wm) = (int(camera[0]), int(camera[1])), (int(model[0]), int(model[1]))
    if Hm > Hc or Wm > Wc:
        raise ValueError('the model size %d x %d is larger than the camera size %d x %d (images are only shrunk)'
                         % (Hm, Wm, Hc, Wc))
    if Hc * Wm != Wc * Hm:
        raise ValueError('camera size %d x %d and model size %d x %d have different aspect ratios' % (Hc, Wc, Hm, Wm))
