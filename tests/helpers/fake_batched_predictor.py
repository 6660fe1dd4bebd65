"""The fake NumPy predictor with the fused ``score`` entry point and ``score_batch``: a batch of G problems is scored by its
own ``score``, one problem after the other, so a planner that batches must hand every controller exactly the scores the
controller's own ``score`` call would have given it.  ``fetch_pixel_distributions(g * M + i)`` returns row ``i`` of problem
``g`` of the last batch (of the last ``score`` call: ``g = 0``)."""
import numpy as np

from oracle import pixel_cost
from tests.helpers.fake_predictor import make_fake_predictor_class


def make_fake_batched_predictor_class(T, height, width, ncam=1, n_context=2):
    Base = make_fake_predictor_class(T, height, width, ncam=ncam, n_context=n_context)

    class FakeBatchedPredictor(Base):
        batches = []        # (G, M) of every score_batch call of the class
        instances = []

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            Base.__init__(self, model_path, hparams, n_gpus=n_gpus, first_gpu=first_gpu)
            type(self).instances.append(self)
            self.n_cam = ncam
            self._resident = None

        def score(self, context, inputs, goal_pix, finalweight=10., only_take_first_view=False):
            out = Base.__call__(self, context, inputs)
            self._resident = out['predicted_pixel_distributions']
            return pixel_cost.eval_pixel_cost(self._resident, np.asarray(goal_pix), finalweight, only_take_first_view)

        def score_batch_refusal(self):
            return None

        def score_batch(self, contexts, inputs, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
            actions = np.asarray(inputs['actions'])
            G, M = actions.shape[:2]
            assert len(contexts) == G and np.asarray(goal_pix).shape[0] == G and task_weights is None
            assert G * M <= self.hparams['run_batch_size'], 'all rows of a batch stay resident in one chunk'
            type(self).batches.append((G, M))
            parts, resident = [], []
            for g in range(G):
                parts.append(self.score(contexts[g], {'actions': actions[g]}, np.asarray(goal_pix)[g], finalweight,
                                        only_take_first_view))
                resident.append(self._resident)
            self._resident = np.concatenate(resident)
            return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])

        def fetch_pixel_distributions(self, sample_index):
            return self._resident[sample_index].copy()

    return FakeBatchedPredictor
