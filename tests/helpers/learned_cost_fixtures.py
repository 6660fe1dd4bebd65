"""Seeded stand-ins that ``tools/make_golden_learned_cost.py`` drives the reference's learned-cost controllers with, and
that ``tests/test_learned_cost.py`` regenerates from the recorded seeds: a fake video predictor with the reference's
``predictor(input_images=, input_state=, input_actions=, input_one_hot_images=)`` call, a fake success classifier and a
fake embedding model.  All NumPy; the "networks" are one seeded matrix on the mean colour of an image.  They return
float64 so that the reference's cost arithmetic around them runs in float64 and can be pinned to round-off."""
import numpy as np


def case_inputs(seed, ncam, H, W, M, T, adim, sdim, n_context):
    rs = np.random.RandomState(seed)
    return {
        'images': rs.randint(0, 256, (n_context + 1, ncam, H, W, 3)).astype(np.uint8),
        'state': rs.normal(0, 0.1, (n_context + 1, sdim)),
        'goal_image': rs.uniform(0, 1, (2, ncam, H, W, 3)).astype(np.float32),
        'actions': rs.normal(0, 0.3, (M, T, adim)),
        'chosen_actions': [rs.normal(0, 0.1, adim) for _ in range(n_context)],
    }


def fake_frames(seed, actions, T, ncam, H, W):
    """Predicted frames ``[b, T, ncam, H, W, 3]`` float32 in [0, 1]: a seeded base video whose brightness follows the
    running sum of the last ``T`` actions' first channel."""
    rs = np.random.RandomState(seed + 77)
    base = rs.uniform(0.05, 0.95, (T, ncam, H, W, 3))
    a = np.asarray(actions, dtype=np.float64)[:, -T:, 0]
    gain = 0.55 + 0.4 * np.tanh(np.cumsum(a, axis=1))
    return (base[None] * gain[:, :, None, None, None, None]).astype(np.float32)


def make_reference_predictor(seed, T, ncam, H, W):
    def predictor(input_images=None, input_state=None, input_actions=None, input_one_hot_images=None):
        return fake_frames(seed, input_actions, T, ncam, H, W), None, None
    return predictor


def classifier_logits(seed, images):
    """``images [N, H, W, 3]`` in [0, 1] -> float32 logits ``[N, 2]``."""
    w = np.random.RandomState(seed + 5).uniform(-3, 3, (3, 2))
    feat = np.asarray(images, dtype=np.float64).mean(axis=(1, 2))
    return (feat @ w).astype(np.float32)


def make_classifier(seed):
    """The reference's ``scoring_func(images)['logits']`` holds POST-softmax values (classifier_controller.py:99-102)."""
    def scoring_func(images):
        z = classifier_logits(seed, images).astype(np.float64)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return {'logits': e / e.sum(axis=1, keepdims=True)}
    return scoring_func


def embed_frames(seed, images, D=8):
    """``images [N, H, W, 3]`` in 0..255 -> float32 embeddings ``[N, D]`` (positive: no cancellation in the inner product)."""
    w = np.random.RandomState(seed + 6).uniform(0.1, 1.0, (3, D))
    return ((np.asarray(images, dtype=np.float64).mean(axis=(1, 2)) / 255.) @ w).astype(np.float32)


def embed_goal(seed, goal, start, D=8):
    """``goal`` / ``start [1, H, W, 3]`` in 0..255 -> float32 ``[1, D]``."""
    w = np.random.RandomState(seed + 7).uniform(0.1, 1.0, (6, D))
    pair = np.concatenate([np.asarray(goal, dtype=np.float64), np.asarray(start, dtype=np.float64)], axis=-1)
    return ((pair.mean(axis=(1, 2)) / 255.) @ w).astype(np.float32)


def make_embedder(seed):
    def scoring_func(goal, start, images):
        return {'goal_enc': embed_goal(seed, goal, start).astype(np.float64),
                'input_enc': embed_frames(seed, images).astype(np.float64)}
    return scoring_func
