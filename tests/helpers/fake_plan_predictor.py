"""A deterministic stand-in predictor whose frames AND distributions depend on the actions, for the plan-page fixtures.

Like ``fake_predictor.py`` it is used on both sides of a golden: ``tools/make_golden_plan_page.py`` plugs it into the
stub-imported reference controller, the tests plug it into this repository's controllers.  Outputs are a pure NumPy
function of (context, actions): nothing but the recorded actions has to travel.  Frames lie in [0, 1] and are float32,
distributions are positive, un-normalised float32 blobs that follow the cumulated actions.
"""
import numpy as np


def make_fake_plan_predictor_class(T, height, width, ncam=1, n_context=2):
    class FakePlanPredictor(object):
        wants_agent_params = False
        n_context_default = n_context
        n_cam = ncam
        actions_seen = []

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            self.hparams = dict(hparams)
            self.n_context = n_context
            self.sequence_length = T + n_context

        def restore(self):
            pass

        def __call__(self, context, inputs):
            actions = np.asarray(inputs['actions'], dtype=np.float64)
            M = actions.shape[0]
            assert actions.shape[1] == T
            type(self).actions_seen.append(actions.copy())
            ctx = np.asarray(context['context_pixel_distributions'])
            ndesig = ctx.shape[-1]
            last = np.asarray(context['context_frames'])[-1].astype(np.float64) / 255.     # [ncam, H, W, 3]
            rr = np.arange(height, dtype=np.float64)[:, None]
            cc = np.arange(width, dtype=np.float64)[None, :]
            path = np.cumsum(actions[:, :, :2], axis=1) * 12.0                             # [M, T, 2]
            distrib = np.zeros((M, T, ncam, height, width, ndesig), dtype=np.float32)
            frames = np.zeros((M, T, ncam, height, width, 3), dtype=np.float32)
            for c in range(ncam):
                for p in range(ndesig):
                    start = np.unravel_index(np.argmax(ctx[-1, c, :, :, p]), (height, width))
                    pr = start[0] + path[:, :, 0] * (1 + c) + p
                    pc = start[1] + path[:, :, 1] - c
                    d2 = (rr[None, None] - pr[:, :, None, None]) ** 2 + (cc[None, None] - pc[:, :, None, None]) ** 2
                    distrib[:, :, c, :, :, p] = ((1.0 + p) * np.exp(-d2 / 6.0) + 1e-3).astype(np.float32)
                wave = 0.5 + 0.5 * np.sin(0.7 * rr[None, None] + path[:, :, 0, None, None] +
                                          0.4 * cc[None, None] * (1 + c) + path[:, :, 1, None, None])
                for ch in range(3):
                    mix = 0.25 + 0.2 * ch
                    frames[:, :, c, :, :, ch] = (mix * last[c, :, :, ch][None, None] + (1.0 - mix) * wave).astype(np.float32)
            return {'predicted_frames': frames, 'predicted_pixel_distributions': distrib}

    return FakePlanPredictor
