"""``fake_frame_predictor.py``'s stand-in with a ``frames_only`` switch: a frames-only instance refuses a context that carries
``context_pixel_distributions`` (as ``HipVPredEvaluation`` does for ``designated_pixel_count`` 0) and returns
``predicted_pixel_distributions: None``; the other is the base fake, which wants them.  Pure NumPy, no ``score_*`` methods,
so a controller drives it through the host path - the path on which the controllers add their centre distribution."""
from tests.helpers.fake_frame_predictor import make_fake_frame_predictor_class


def make_fake_frames_only_predictor_class(T, height, width, ncam=1, n_context=2, frames_only=True):
    base = make_fake_frame_predictor_class(T, height, width, ncam=ncam, n_context=n_context)

    class FakeFramesOnlyPredictor(base):
        supports_frames_only = True

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            super(FakeFramesOnlyPredictor, self).__init__(model_path, hparams, n_gpus=n_gpus, first_gpu=first_gpu)
            self.frames_only = frames_only

        def __call__(self, context, inputs):
            has = context.get('context_pixel_distributions') is not None
            if self.frames_only and has:
                raise ValueError('frames-only predictor: the context must not carry context_pixel_distributions')
            if not self.frames_only and not has:
                raise KeyError('context_pixel_distributions')
            out = super(FakeFramesOnlyPredictor, self).__call__(context, inputs)
            if self.frames_only:
                out['predicted_pixel_distributions'] = None
            return out

    return FakeFramesOnlyPredictor


def assert_same_messages(a, b):
    """Two plan-page message streams ``[(kind, path, payload), ...]`` carry the same files with the same bytes."""
    import numpy as np
    assert len(a) == len(b) and len(a) > 0
    for (kind_a, path_a, pay_a), (kind_b, path_b, pay_b) in zip(a, b):
        assert (kind_a, path_a) == (kind_b, path_b)
        if isinstance(pay_a, np.ndarray):
            np.testing.assert_array_equal(pay_a, pay_b)
        else:
            assert pay_a == pay_b
