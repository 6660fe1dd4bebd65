"""Designated-pixel registration arithmetic (host NumPy).

Restates the cost-side math of the reference's
``visual_mpc/policy/cem_controllers/register_gtruth_controller.py`` (``register_gtruth`` :54-111,
``get_warp_err`` :113-173): given a warp field that maps the current frame onto a reference
frame (the first frame of the episode and/or the goal image), re-localise every designated pixel
in the current frame and derive per-(camera, registration) trade-off weights from the warp error.

The registration *network* (``visual_mpc.registration_network``, ``:7,32``) is not part of the
reference snapshot; this project ships its own (``video_prediction/registration_net.py``:
``HipRegistrationNet`` on the device, ``HostRegistrationNet`` on the CPU).  The warper stays a
plug-in, so any other source of a flow field fits too:

    warper(current [ncam,H,W,3] float32, reference [ncam,H,W,3] float32)
        -> warped [ncam,H,W,3], flow (ignored), warp_pts [ncam,H,W,2]

``warp_pts[c, r, col]`` holds the (x, y) = (col, row) position in the *current* frame that
corresponds to reference pixel (r, col) - the reference flips it to (row, col) (``:132-135``).
"""
import numpy as np


def region_bounds(center, width, limit_rows, limit_cols, inclusive_limit):
    """[lo, hi) row and column ranges of the (2*width+1)^2 window around ``center`` (row, col).

    The reference clips the start window to ``size - 1`` (``:142-143``) and the goal window to
    ``size`` (``:152-153``); ``inclusive_limit`` selects which.
    """
    hi_r = limit_rows - 1 if inclusive_limit else limit_rows
    hi_c = limit_cols - 1 if inclusive_limit else limit_cols
    r = np.clip(np.array((center[0] - width, center[0] + width + 1)), 0, hi_r)
    c = np.clip(np.array((center[1] - width, center[1] + width + 1)), 0, hi_c)
    return r, c


def get_warp_err(icam, pix_t0, goal_pix, start_image, goal_image, start_warp_pts, goal_warp_pts,
                 warped_image_start, warped_image_goal, register_gtruth=('start', 'goal'),
                 register_region=False, pred_height=None):
    """Tracked pixel and warp error of every task for one camera.

    pix_t0, goal_pix: [ntask, 2] (row, col) of the designated pixel in the first frame / of the
    goal pixel in the goal image.  Returns ``warperrs [ntask, nreg]`` and ``desig [ntask, nreg, 2]``
    (row, col) in the current frame.  ``register_region`` takes the median flow and the mean
    squared photometric error over a window (half-width 2 below 96 rows, else 5, ``:139-141``);
    otherwise the flow and the L2 photometric error at the single pixel (``:129-135,163-170`` - dead code
    in the reference, whose point mode leaves the errors zero; see ``oracle/registration.py``).
    ``pred_height``: the predictor's image height when it differs from the images' (``:172``).
    Pinned to the reference's own outputs by ``tests/golden/registration.npz``.
    """
    H, W = start_image.shape[1:3]
    nreg = len(register_gtruth)
    ntask = len(pix_t0)
    warperrs = np.zeros((ntask, nreg))
    desig = np.zeros((ntask, nreg, 2))
    refs = []
    if 'start' in register_gtruth:
        refs.append((pix_t0, start_image, start_warp_pts, warped_image_start, True))
    if 'goal' in register_gtruth:
        refs.append((goal_pix, goal_image, goal_warp_pts, warped_image_goal, False))
    width = 5 if H >= 96 else 2
    for p in range(ntask):
        for r, (pix, ref_img, warp_pts, warped, is_start) in enumerate(refs):
            pr, pc = int(pix[p][0]), int(pix[p][1])
            if register_region:
                rr, cc = region_bounds((pr, pc), width, H, W, inclusive_limit=is_start)
                win = (slice(rr[0], rr[1]), slice(cc[0], cc[1]))
                warperrs[p, r] = np.mean(np.square(ref_img[icam][win] - warped[icam][win]))
                field = warp_pts[icam][win]
                desig[p, r] = (np.median(field[:, :, 1]), np.median(field[:, :, 0]))      # (x,y) -> (row,col)
            else:
                warperrs[p, r] = np.linalg.norm(ref_img[icam][pr, pc] - warped[icam][pr, pc])
                desig[p, r] = np.flip(warp_pts[icam][pr, pc], 0)
    if pred_height is not None:
        desig = desig * pred_height / H
    return warperrs, desig


def medium_res_pixels(pix, image_height, img_height):
    """Pixels in the model's coordinates -> the agent's (medium-resolution) table the registration runs on: the
    reference's ``(pix * agentparams['image_height'] / self._img_height).astype(np.int)`` (``:183,191``), truncation
    included.  One ratio for rows and columns."""
    return (np.asarray(pix) * image_height / img_height).astype(int)


def model_res_pixels(desig, img_height, image_height):
    """Tracked pixels in the agent's coordinates -> the model's: ``desig * self._img_height / agentparams['image_height']``
    (``:172``), not rounded."""
    return np.asarray(desig) * img_height / image_height


def tradeoff_weights(warperrs):
    """``warperrs [ncam, ntask, nreg]`` -> weights of the same shape, each task's summing to 1.

    weight = (1/err) / sum over (camera, registration) of (1/err)   (reference ``:88-91``).
    """
    inv = 1.0 / warperrs
    return inv / np.sum(np.sum(inv, 0, keepdims=True), 2, keepdims=True)


def bilinear_warp(current, flow):
    """``current [ncam, H, W, 3]``, ``flow [ncam, H, W, 2]`` (dx, dy) -> ``(warped, warp_pts)``: the frame sampled
    bilinearly at ``warp_pts[c, r, col] = (col + dx, r + dy)``, border-clamped.  Vectorised; the same float32
    operations in the same order as ``oracle.registration.bilinear_warp_loops`` and ``bilinear_clamped`` of
    ``csrc/vf_small_kernels.h``, so all three agree bit for bit."""
    cur = np.asarray(current, dtype=np.float32)
    fl = np.asarray(flow, dtype=np.float32)
    ncam, H, W = cur.shape[:3]
    f32, f64 = np.float32, np.float64
    x = np.arange(W, dtype=f32)[None, None, :] + fl[..., 0]
    y = np.arange(H, dtype=f32)[None, :, None] + fl[..., 1]
    pts = np.stack([x, y], axis=-1).astype(f32)
    xc = np.minimum(np.maximum(x, f32(0)), f32(W - 1))
    yc = np.minimum(np.maximum(y, f32(0)), f32(H - 1))
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx = (xc - x0.astype(f32)).astype(f32).astype(f64)[..., None]
    fy = (yc - y0.astype(f32)).astype(f32).astype(f64)[..., None]
    cam = np.arange(ncam)[:, None, None]
    a, b = cur[cam, y0, x0].astype(f64), cur[cam, y0, x1].astype(f64)
    c, d = cur[cam, y1, x0].astype(f64), cur[cam, y1, x1].astype(f64)

    def lerp(t, lo, hi):        # fmaf(t, hi - lo, lo): the difference rounded to float32, the fma exact then rounded
        return (t * (hi - lo).astype(f32).astype(f64) + lo).astype(f32).astype(f64)

    top, bot = lerp(fx, a, b), lerp(fx, c, d)
    return lerp(fy, top, bot).astype(f32), pts
