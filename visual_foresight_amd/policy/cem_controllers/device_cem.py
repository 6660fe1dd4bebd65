"""The device side of ``PhiloxGaussianCEMSampler``: buffers and launches of ``vf_cem_refit`` / ``vf_cem_sample``.

``DeviceCEM`` owns the workspace (the proposal in factor form) and the per-iteration candidate, elite and trial buffers of
one controller, all allocated once.  Every method only enqueues on the current stream of its device; ``download`` is the one
synchronisation of a planning call.  PyTorch carries the buffers, the arithmetic is ``csrc/vf_cem.h``.
"""
import ctypes

import numpy as np

from visual_foresight_amd import _lib

HEADER_BYTES = 16


def cem_config(sampler, n_elites, append_action=None):
    """The ``vf_cem_config`` of a ``PhiloxGaussianCEMSampler`` (its limits, key and post-processing switches)."""
    hp, adim = sampler._hp, sampler._adim
    tail = [float(v) for v in (append_action or ())]
    rej, trunc, discrete = sampler.limits()
    cfg = _lib.VfCemConfig()
    cfg.nactions, cfg.repeat, cfg.adim, cfg.tail = int(hp.nactions), int(hp.repeat), int(adim), len(tail)
    cfg.n_elites = int(n_elites)
    cfg.max_trials = int(hp.max_trials) if hp.rejection_sampling else 1
    cfg.rejection = int(bool(hp.rejection_sampling))
    cfg.zero_first = int(bool(hp.add_zero_action and not hp.rejection_sampling))
    cfg.discrete_mask = int(sum(1 << int(c) for c in np.flatnonzero(discrete)))
    cfg.seed_lo, cfg.seed_hi = sampler.key
    for i in range(8):
        cfg.rej_lim[i] = float(rej[i]) if i < adim else float('inf')
        cfg.trunc_lim[i] = float(trunc[i]) if i < adim else float('inf')
        cfg.tail_value[i] = tail[i] if i < len(tail) else 0.0
    return cfg


def workspace_image(mean, A, rmax):
    """``(R, mean [D], A [D, R])`` as the bytes of a workspace whose ``A`` has room for ``rmax`` columns."""
    D, R = A.shape
    head = np.zeros(4, dtype=np.int32)
    head[0] = R
    body = np.zeros((1 + rmax, D), dtype=np.float64)
    body[0] = mean
    body[1:1 + R] = A.T
    return np.concatenate((head.view(np.uint8), body.reshape(-1).view(np.uint8)))


def read_workspace(image, D):
    """Workspace bytes (NumPy uint8) -> ``(R, mean [D], A [D, R])``."""
    image = np.ascontiguousarray(image)
    R = int(image[:HEADER_BYTES].view(np.int32)[0])
    body = image[HEADER_BYTES:].view(np.float64).reshape(-1, D)
    return R, body[0].copy(), body[1:1 + R].T.copy()


class DeviceCEM(object):
    def __init__(self, sampler, n_elites, n_iter, max_samples, device, append_action=None):
        import torch
        self._torch = torch
        self.device = torch.device(device)
        self._lib = _lib.load_library()
        self.cfg = cem_config(sampler, n_elites, append_action)
        hp = sampler._hp
        self.D, self.K = int(hp.nactions) * sampler._adim, int(n_elites)
        self.T, self.W = int(hp.nactions) * int(hp.repeat), sampler._adim + self.cfg.tail
        self.n_iter, self.max_samples = int(n_iter), int(max_samples)
        nbytes = self._lib.vf_cem_workspace_bytes(ctypes.byref(self.cfg))
        if nbytes == 0:
            raise ValueError('device CEM: %s' % self._lib.vf_last_error().decode())
        self.rmax = max(self.D, self.K)
        dev = self.device
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros((self.n_iter, self.max_samples, self.T, self.W), dtype=torch.float32, device=dev)
        self.scores = torch.zeros((self.n_iter, self.max_samples), dtype=torch.float64, device=dev)
        self.elite_index = torch.zeros((self.n_iter, self.K), dtype=torch.int32, device=dev)
        self.elite_score = torch.zeros((self.n_iter, self.K), dtype=torch.float64, device=dev)
        self.elite_plans = torch.zeros((self.K, self.T, self.W), dtype=torch.float32, device=dev)
        self.trials = torch.zeros((self.n_iter, self.max_samples), dtype=torch.int32, device=dev)
        self.capped = torch.zeros((self.n_iter, self.max_samples), dtype=torch.int32, device=dev)
        self._staging = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def upload(self, mean, A):
        """Make ``(mean, A [D, R])`` the proposal: one asynchronous copy of the workspace image."""
        image = workspace_image(np.asarray(mean, np.float64), np.asarray(A, np.float64), self.rmax)
        # (the pinned stage may still feed the previous call's copy: wait for that one, it is long done)
        self._torch.cuda.current_stream(self.device).synchronize()
        self._staging.numpy()[:] = image
        self.workspace.copy_(self._staging, non_blocking=True)

    def sample(self, itr, M, call):
        """Candidates of iteration ``itr`` -> the device tensor ``[M, T, adim + tail]`` the rollout reads."""
        out = self.actions[itr, :M]
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_sample(self.device.index, ctypes.byref(self.cfg), self.workspace.data_ptr(), int(call),
                                               int(M), out.data_ptr(), self.trials[itr].data_ptr(),
                                               self.capped[itr].data_ptr(), self._stream()))
        return out

    def refit(self, itr, scores_dev, actions_dev):
        """Elites of ``scores_dev [M]`` (float64) over ``actions_dev [M, T, adim + tail]``, and the refit into the workspace."""
        M = int(scores_dev.shape[0])
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_refit(self.device.index, ctypes.byref(self.cfg), scores_dev.data_ptr(),
                                              actions_dev.data_ptr(), M, self.elite_index[itr].data_ptr(),
                                              self.elite_score[itr].data_ptr(), self.elite_plans.data_ptr(),
                                              self.workspace.data_ptr(), self._stream()))

    def read_proposal(self):
        """(synchronises) -> ``(R, mean, A [D, R])`` of the workspace."""
        return read_workspace(self.workspace.cpu().numpy(), self.D)
