"""NumPy restatement of the goal-image cost (reference ``visual_mpc/policy/cem_controllers/goal_im_controller.py:93``:
``((gen_images[:, -1, 0] - goalims) ** 2).mean((1, 2, 3))``) with the modes of ``vf_goal_image_scores``, in float64.
Test infrastructure only."""
import numpy as np


def goal_image_scores(frames, goal, steps='last', finalweight=10., first_view_only=False, n_draws=1):
    """frames ``[B, T, ncam, H, W, 3]`` (B = actions * n_draws, draw-minor), goal ``[ncam, H, W, 3]`` ->
    (scores [A], per_view [A, ncam], cost_per_step [A, ncam, T])."""
    f = np.asarray(frames, dtype=np.float64)
    g = np.asarray(goal, dtype=np.float64)
    B, T, ncam = f.shape[:3]
    mse = ((f - g[None, None]) ** 2).mean(axis=(3, 4, 5)).transpose(0, 2, 1)           # [B, ncam, T]
    if steps == 'last':
        e = mse[:, :, -1]
    elif steps == 'weighted':
        w = np.ones(T)
        w[-1] = finalweight
        e = (mse * w).sum(axis=2) / w.sum()
    else:
        raise ValueError(steps)
    A = B // n_draws
    e = e.reshape(A, n_draws, ncam).mean(axis=1)
    cps = mse.reshape(A, n_draws, ncam, T).mean(axis=1)
    scores = e[:, 0].copy() if first_view_only else e.mean(axis=1)
    return scores, e, cps
