"""A deterministic stand-in for the action-inference predictor of the inverse-model policy.

Used on BOTH sides of ``tests/golden/inverse_model.*``: ``tools/make_golden.py`` plugs it into the stub-imported reference
controller, the tests plug it into this repo's controller.  Its actions are a pure function of a checksum of its inputs,
and it records shape, dtype and checksum of every argument, so the two runs can be compared call by call.
"""
import numpy as np


def checksum(x):
    """Position-weighted float64 sum: sensitive to the values, their order and the dtype-dependent rounding."""
    v = np.asarray(x, dtype=np.float64).ravel()
    return float(np.dot(v, 1.0 + (np.arange(v.size) % 251) / 251.0))


def make_fake_action_inference(n_actions, adim):
    class FakeActionInference(object):
        instances = []

        def __init__(self, model_params_path, hparams, n_gpus=1, first_gpu=0):
            self.model_params_path, self.hparams = model_params_path, dict(hparams)
            self.n_gpus, self.first_gpu = n_gpus, first_gpu
            self.restored = 0
            self.calls = []
            type(self).instances.append(self)

        def restore(self):
            self.restored += 1

        def __call__(self, start_image, goal_image, context_actions, context_frames):
            args = (start_image, goal_image, context_actions, context_frames)
            rec = [{'shape': list(np.shape(a)), 'dtype': str(np.asarray(a).dtype), 'checksum': checksum(a)} for a in args]
            self.calls.append(rec)
            phase = sum(r['checksum'] for r in rec)
            t = np.arange(n_actions, dtype=np.float64)[:, None]
            d = np.arange(adim, dtype=np.float64)[None, :]
            return (0.05 * np.sin(phase + 0.7 * t + 1.3 * d))[None].astype(np.float32)

    return FakeActionInference
