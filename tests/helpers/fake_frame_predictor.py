"""A deterministic stand-in video predictor whose predicted FRAMES depend on the actions (``fake_predictor.py`` moves
distributions and returns black frames): a bright blob travels over a dimmed copy of the last context frame.  Pure
NumPy function of (context, actions); ``VPredEvaluation`` duck-type without ``score`` / ``score_goal_image``."""
import numpy as np


def make_fake_frame_predictor_class(T, height, width, ncam=1, n_context=2):
    class FakeFramePredictor(object):
        wants_agent_params = False
        n_context_default = n_context

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            self.hparams = dict(hparams)
            self.n_context = n_context
            self.sequence_length = T + n_context
            self.n_cam = ncam
            self.contexts = []          # key -> shape of every context it was called with
            self.actions_seen = []      # the candidate actions of every call

        def restore(self):
            pass

        def __call__(self, context, inputs):
            actions = np.asarray(inputs['actions'], dtype=np.float64)
            M = actions.shape[0]
            assert actions.shape[1] == T
            self.contexts.append({k: np.asarray(v).shape for k, v in context.items()})
            self.actions_seen.append(actions.copy())
            base = np.asarray(context['context_frames'])[-1].astype(np.float64) / 255.          # [ncam, H, W, 3]
            rr = np.arange(height, dtype=np.float64)[:, None]
            cc = np.arange(width, dtype=np.float64)[None, :]
            path = np.cumsum(actions[:, :, :2], axis=1) * 30.0
            frames = np.zeros((M, T, ncam, height, width, 3), dtype=np.float32)
            for c in range(ncam):
                pr = height / 2. + path[:, :, 0] * (1 + c)
                pc = width / 2. + path[:, :, 1] - c
                d2 = (rr[None, None] - pr[:, :, None, None]) ** 2 + (cc[None, None] - pc[:, :, None, None]) ** 2
                blob = np.exp(-d2 / 12.0)[..., None] * np.array([1.0, 0.6, 0.3 + 0.2 * c])
                frames[:, :, c] = np.clip(0.4 * base[c][None, None] + blob, 0., 1.).astype(np.float32)
            distrib = np.full((M, T, ncam, height, width, 1), 1.0 / (height * width), dtype=np.float32)
            return {'predicted_frames': frames, 'predicted_pixel_distributions': distrib}

    return FakeFramePredictor
