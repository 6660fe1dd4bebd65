"""The device side of the four Philox samplers: buffers and launches of ``vf_cem_refit`` / ``vf_cem_sample``
(``DeviceCEM``, for ``PhiloxGaussianCEMSampler``), of ``vf_cem_soft_refit`` / ``vf_cem_sample_corr``
(``DeviceCorrelatedCEM``, for ``PhiloxCorrelatedNoiseSampler``), of ``vf_cem_refit`` / ``vf_cem_sample_fold``
(``DeviceFoldingCEM``, for ``PhiloxFoldingCEMSampler``) and of ``vf_cem_refit`` / ``vf_cem_sample_autograsp``
(``DeviceAutograspCEM``, for ``PhiloxAutograspSampler``).

A driver owns the workspace (the proposal) and the per-iteration candidate and elite buffers of one controller, all
allocated once.  Every method only enqueues on the current stream of its device; the controller's one download is the one
synchronisation of a planning call.  PyTorch carries the buffers, the arithmetic is ``csrc/vf_cem.h``.  The controller
drives either through ``begin`` / ``sample`` / ``refit`` / ``downloads`` / ``finish`` (a sampler names its driver:
``device_cem_driver``).

Who owns what.  ``_Driver``: the device and library handles, ``_stream``, the buffers every driver has, the workspace-size
query, the refit call under ``refit_cfg`` and, for the factor-form proposal ``(R, mean, A)`` of the Gaussian, folding and
autograsp drivers, ``upload`` through the pinned stage and ``read_proposal``.  A driver adds ``configure`` (its configs),
``begin`` / ``finish`` and ``sample``.  ``DeviceCEM`` also has ``trials`` / ``capped`` and downloads them;
``DeviceAutograspCEM``, a ``DeviceCEM``, adds ``share``.  ``DeviceCorrelatedCEM`` keeps its own workspace layout, and with
it ``upload`` (no stage), the size and refit entries it names, ``_steps`` and ``read_proposal``.
"""
import ctypes

import numpy as np

from visual_foresight_amd import _lib

HEADER_BYTES = 16


def _fill_tail(cfg, append_action):
    """``tail`` / ``tail_value`` of a config: the constants appended to every action row."""
    tail = [float(v) for v in (append_action or ())]
    cfg.tail = len(tail)
    for i in range(8):
        cfg.tail_value[i] = tail[i] if i < len(tail) else 0.0


def cem_config(sampler, n_elites, append_action=None):
    """The ``vf_cem_config`` of a ``PhiloxGaussianCEMSampler`` (its limits, key and post-processing switches)."""
    hp, adim = sampler._hp, sampler._adim
    rej, trunc, discrete = sampler.limits()
    cfg = _lib.VfCemConfig()
    cfg.nactions, cfg.repeat, cfg.adim = int(hp.nactions), int(hp.repeat), int(adim)
    _fill_tail(cfg, append_action)
    cfg.n_elites = int(n_elites)
    cfg.max_trials = int(hp.max_trials) if hp.rejection_sampling else 1
    cfg.rejection = int(bool(hp.rejection_sampling))
    cfg.zero_first = int(bool(hp.add_zero_action and not hp.rejection_sampling))
    cfg.discrete_mask = int(sum(1 << int(c) for c in np.flatnonzero(discrete)))
    cfg.seed_lo, cfg.seed_hi = sampler.key
    for i in range(8):
        cfg.rej_lim[i] = float(rej[i]) if i < adim else float('inf')
        cfg.trunc_lim[i] = float(trunc[i]) if i < adim else float('inf')
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


class _Driver(object):
    size_entry, refit_entry = 'vf_cem_workspace_bytes', 'vf_cem_refit'      # (the library's, under refit_cfg)

    def __init__(self, sampler, n_elites, n_iter, max_samples, device, append_action=None):
        import torch
        self._torch = torch
        self.device = torch.device(device)
        self._lib = _lib.load_library()
        self.K, self.n_iter, self.max_samples = int(n_elites), int(n_iter), int(max_samples)
        self.configure(sampler, self.max_samples, append_action)
        rc = self.refit_cfg             # (the config of workspace and refit)
        self.D, self.W = rc.nactions * rc.adim, rc.adim + rc.tail
        self.T = self._steps(rc)
        nbytes = getattr(self._lib, self.size_entry)(ctypes.byref(rc))
        if nbytes == 0:
            raise ValueError('device CEM: %s' % self._lib.vf_last_error().decode())
        self.workspace = self._zeros(nbytes, torch.uint8)
        self.actions = self._zeros((self.n_iter, self.max_samples, self.T, self.W), torch.float32)
        self.scores = self._zeros((self.n_iter, self.max_samples), torch.float64)
        self.elite_index = self._zeros((self.n_iter, self.K), torch.int32)
        self.elite_score = self._zeros((self.n_iter, self.K), torch.float64)
        self.elite_plans = self._zeros((self.K, self.T, self.W), torch.float32)
        self._staging = self._stage(nbytes)

    def _steps(self, cfg):
        """Rows of a plan: every action held ``repeat`` steps."""
        return cfg.nactions * cfg.repeat

    def _stage(self, nbytes):
        """The pinned host image ``upload`` copies the workspace from."""
        return self._torch.zeros(nbytes, dtype=self._torch.uint8).pin_memory()

    def _zeros(self, shape, dtype):
        return self._torch.zeros(shape, dtype=dtype, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def downloads(self, M):
        """What the call's one download carries besides scores, elite indices and the final elite plans."""
        return []

    def upload(self, mean, A):
        """Make ``(mean, A [D, R])`` the proposal: one asynchronous copy of the workspace image."""
        image = workspace_image(np.asarray(mean, np.float64), np.asarray(A, np.float64), max(self.D, self.K))
        # (the pinned stage may still feed the previous call's copy: wait for that one, it is long done)
        self._torch.cuda.current_stream(self.device).synchronize()
        self._staging.numpy()[:] = image
        self.workspace.copy_(self._staging, non_blocking=True)

    def refit(self, itr, scores_dev, actions_dev):
        """Elites of ``scores_dev [M]`` (float64) over ``actions_dev [M, T, W]``, and the refit into the workspace."""
        entry = getattr(self._lib, self.refit_entry)
        M = int(scores_dev.shape[0])
        with self._torch.cuda.device(self.device):
            _lib.check(entry(self.device.index, ctypes.byref(self.refit_cfg), scores_dev.data_ptr(), actions_dev.data_ptr(), M,
                             self.elite_index[itr].data_ptr(), self.elite_score[itr].data_ptr(), self.elite_plans.data_ptr(),
                             self.workspace.data_ptr(), self._stream()))

    def read_proposal(self):
        """(synchronises) -> ``(R, mean, A [D, R])`` of the workspace."""
        return read_workspace(self.workspace.cpu().numpy(), self.D)


class DeviceCEM(_Driver):
    config = staticmethod(cem_config)       # (sampler, n_elites, append_action) -> the vf_cem_config of workspace and refit

    def __init__(self, sampler, n_elites, n_iter, max_samples, device, append_action=None):
        super(DeviceCEM, self).__init__(sampler, n_elites, n_iter, max_samples, device, append_action)
        self.trials = self._zeros((self.n_iter, self.max_samples), self._torch.int32)
        self.capped = self._zeros((self.n_iter, self.max_samples), self._torch.int32)

    def configure(self, sampler, M, append_action):
        self.cfg = self.refit_cfg = self.config(sampler, self.K, append_action)

    # ------------------------------------------------------------------ one planning call, as the controller drives it
    def begin(self, sampler, t, M, append_action=None, state=None):
        """Start a planning call at time ``t`` that draws ``M`` sequences per iteration: the sampler's first proposal.
        ``state``: the state row the call starts from (the folding driver reads it)."""
        self.configure(sampler, M, append_action)           # (reset() makes a new sampler: its key)
        self._mean0, std = sampler.initial_proposal(t)
        assert sampler.draws_for(self.max_samples) == M
        self.upload(self._mean0, np.diag(std))

    def downloads(self, M):
        return [self.trials[:, :M], self.capped[:, :M]]

    def finish(self, sampler, extras):
        """The sampler's diagnostics and state after the download (``extras``: ``downloads`` on the host)."""
        trials, capped = extras
        sampler.last_trials, sampler.last_capped = trials[-1].astype(np.int32), capped[-1] != 0
        sampler.n_capped += int(capped.sum())
        sampler._mean, sampler._A = self._mean0, None       # (the fitted proposal stays on the device)

    def sample(self, itr, M, call):
        """Candidates of iteration ``itr`` -> the device tensor ``[M, T, adim + tail]`` the rollout reads."""
        out = self.actions[itr, :M]
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_sample(self.device.index, ctypes.byref(self.cfg), self.workspace.data_ptr(), int(call),
                                               int(M), out.data_ptr(), self.trials[itr].data_ptr(),
                                               self.capped[itr].data_ptr(), self._stream()))
        return out


# ---------------------------------------------------------------------------------------------------- correlated noise
def corr_workspace_bytes(D, K, refit_cov):
    """Bytes of the workspace of ``vf_cem_soft_refit`` / ``vf_cem_sample_corr`` (header, centre, mean, soft, A)."""
    return HEADER_BYTES + 8 * (2 * D + K + (K * D if refit_cov else 0))


def corr_config(sampler, n_elites, append_action=None):
    """The ``vf_cem_corr_config`` of a ``PhiloxCorrelatedNoiseSampler`` (its scales, key and the filter's first step)."""
    hp, adim = sampler._hp, sampler._adim
    std, bias, first = sampler.std(), sampler.bias(), sampler.first_predecessor()
    cfg = _lib.VfCemCorrConfig()
    cfg.nactions, cfg.adim, cfg.n_elites = int(hp.nactions), int(adim), int(n_elites)
    _fill_tail(cfg, append_action)
    cfg.refit_cov, cfg.has_first_prev = int(bool(hp.refit_cov)), int(first is not None)
    cfg.seed_lo, cfg.seed_hi = sampler.key
    cfg.kappa, cfg.beta_0, cfg.beta_1 = float(hp.kappa), float(hp.beta_0), float(hp.beta_1)
    for i in range(8):
        cfg.std[i] = float(std[i]) if i < adim else 0.0
        cfg.bias[i] = float(bias[i]) if i < adim else 0.0
        cfg.first_prev[i] = float(first[i]) if first is not None and i < adim else 0.0
    return cfg


def read_corr_workspace(image, D, K, refit_cov):
    """Workspace bytes (NumPy uint8) -> dict: ``R``, ``valid``, ``centre [D]``, ``mean [D]``, ``soft [K]``, ``A [D, R]``."""
    image = np.ascontiguousarray(image)
    head = image[:HEADER_BYTES].view(np.int32)
    body = image[HEADER_BYTES:].view(np.float64)
    R = int(head[0])
    A = body[2 * D + K:2 * D + K + R * D].reshape(R, D).T.copy() if refit_cov else np.zeros((D, 0))
    return dict(R=R, valid=bool(head[1]), centre=body[:D].copy(), mean=body[D:2 * D].copy(), soft=body[2 * D:2 * D + K].copy(),
                A=A)


class DeviceCorrelatedCEM(_Driver):
    size_entry, refit_entry = 'vf_cem_corr_workspace_bytes', 'vf_cem_soft_refit'    # (header, centre, mean, soft, A)

    def __init__(self, sampler, n_elites, n_iter, max_samples, device, append_action=None):
        super(DeviceCorrelatedCEM, self).__init__(sampler, n_elites, n_iter, max_samples, device, append_action)
        self.refit_cov = bool(sampler._hp.refit_cov)
        assert self.workspace.numel() == corr_workspace_bytes(self.D, self.K, self.refit_cov)

    def configure(self, sampler, M, append_action):
        self.cfg = self.refit_cfg = corr_config(sampler, self.K, append_action)

    def _steps(self, cfg):
        return cfg.nactions         # (no action is held)

    def _stage(self, nbytes):
        return None                 # (upload only zeroes the header on the device)

    # ------------------------------------------------------------------ one planning call, as the controller drives it
    def begin(self, sampler, t, M, append_action=None, state=None):
        """Start a planning call: the first proposal has no centre, and the filter's first step is the sampler's."""
        self.configure(sampler, M, append_action)           # (reset() makes a new sampler: its key)
        sampler.start_planning_call()
        self.upload()

    def finish(self, sampler, extras):
        sampler.start_planning_call()       # (the fit stays on the device)

    def upload(self):
        """Make "no centre, no factor" the proposal: the workspace's header is zeroed on the stream."""
        self.workspace[:HEADER_BYTES].zero_()

    def sample(self, itr, M, call):
        """Candidates of iteration ``itr`` -> the device tensor ``[M, nactions, adim + tail]`` the rollout reads."""
        out = self.actions[itr, :M]
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_sample_corr(self.device.index, ctypes.byref(self.cfg), self.workspace.data_ptr(),
                                                    int(call), int(M), out.data_ptr(), self._stream()))
        return out

    def read_proposal(self):
        """(synchronises) -> the workspace as ``read_corr_workspace`` gives it."""
        return read_corr_workspace(self.workspace.cpu().numpy(), self.D, self.K, self.refit_cov)


# ---------------------------------------------------------------------------------------------------- folding
def fold_refit_config(sampler, n_elites, append_action=None):
    """The ``vf_cem_config`` under which ``vf_cem_workspace_bytes`` / ``vf_cem_refit`` serve a ``PhiloxFoldingCEMSampler``:
    the Gaussian proposal with ``adim = 4``, nothing rejected, nothing limited."""
    hp = sampler._hp
    cfg = _lib.VfCemConfig()
    cfg.nactions, cfg.repeat, cfg.adim = int(hp.nactions), int(hp.repeat), 4
    _fill_tail(cfg, append_action)
    cfg.n_elites, cfg.max_trials = int(n_elites), 1
    cfg.seed_lo, cfg.seed_hi = sampler.key
    for i in range(8):
        cfg.rej_lim[i] = cfg.trunc_lim[i] = float('inf')
    return cfg


def fold_config(sampler, n_elites, M, append_action=None):
    """The ``vf_cem_fold_config`` of a ``PhiloxFoldingCEMSampler`` whose calls draw ``M`` sequences."""
    hp = sampler._hp
    cfg = _lib.VfCemFoldConfig()
    cfg.nactions, cfg.repeat, cfg.n_elites = int(hp.nactions), int(hp.repeat), int(n_elites)
    _fill_tail(cfg, append_action)
    cfg.n_scripted = int(sampler.check_draws(M))
    cfg.seed_lo, cfg.seed_hi = sampler.key
    start = sampler.start_xy()
    for i in range(2):
        cfg.start_xy[i] = float(start[i])
    for i in range(3):
        cfg.max_shift[i] = float(hp.max_shift[i])
    return cfg


class DeviceFoldingCEM(_Driver):
    def configure(self, sampler, M, append_action):
        self.refit_cfg = fold_refit_config(sampler, self.K, append_action)
        self.cfg = fold_config(sampler, self.K, M, append_action)

    # ------------------------------------------------------------------ one planning call, as the controller drives it
    def begin(self, sampler, t, M, append_action=None, state=None):
        """Start a planning call at time ``t`` from the state row ``state``: the gripper's xy goes into the config, the first
        proposal ``(0, diag(std))`` into the workspace."""
        mean, std = sampler.initial_proposal(t, state)
        self.configure(sampler, M, append_action)           # (reset() makes a new sampler: its key)
        self.upload(mean, np.diag(std))

    def finish(self, sampler, extras):
        pass        # (the fitted proposal stays on the device; the next call starts from the first proposal)

    def sample(self, itr, M, call):
        """Candidates of iteration ``itr`` -> the device tensor ``[M, T, 4 + tail]`` the rollout reads."""
        out = self.actions[itr, :M]
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_sample_fold(self.device.index, ctypes.byref(self.cfg), self.workspace.data_ptr(),
                                                    int(call), int(M), out.data_ptr(), self._stream()))
        return out


# ---------------------------------------------------------------------------------------------------- autograsp
def autograsp_config(sampler, n_elites, append_action=None):
    """The ``vf_cem_config`` of a ``PhiloxAutograspSampler``: its parent's over the moves, the tail led by the gripper column
    (``tail_value[0]`` is not read) with the appended constants behind it."""
    return cem_config(sampler, n_elites, [0.0] + [float(v) for v in (append_action or ())])


def grip_config(sampler, by_share):
    """The ``vf_cem_grip_config`` of a sampling call of a ``PhiloxAutograspSampler``, by height or by the elites' share."""
    hp = sampler._hp
    cfg = _lib.VfCemGripConfig()
    cfg.mode, cfg.reopen = int(bool(by_share)), int(bool(hp.reopen))
    cfg.state_z, cfg.action_norm_factor, cfg.z_thresh = sampler.state_z(), float(hp.action_norm_factor), float(hp.z_thresh)
    cfg.deviation_prob = float(hp.deviation_prob)
    cfg.close_cmd, cfg.open_cmd = float(hp.gripper_close_cmd), float(hp.gripper_open_cmd)
    return cfg


class DeviceAutograspCEM(DeviceCEM):
    """``DeviceCEM`` over the moves; rows of ``[moves | gripper | appended constants]``, and ``share [T]`` as scratch."""
    config = staticmethod(autograsp_config)

    def __init__(self, sampler, n_elites, n_iter, max_samples, device, append_action=None):
        super(DeviceAutograspCEM, self).__init__(sampler, n_elites, n_iter, max_samples, device, append_action)
        self.share = self._zeros(self.T, self._torch.float32)
        self._sampler = sampler

    def begin(self, sampler, t, M, append_action=None, state=None):
        """As ``DeviceCEM.begin``; the height the call starts from, ``state[2]``, goes into the grip config."""
        sampler.start_planning_call(state)
        self._sampler = sampler
        super(DeviceAutograspCEM, self).begin(sampler, t, M, append_action, state)

    def sample(self, itr, M, call):
        """Candidates of iteration ``itr`` -> ``[M, T, adim + 1 + tail]``: by height, or by the share of the elites the last
        ``refit`` left in ``elite_plans`` (``no_refit`` False, from the second iteration on)."""
        out = self.actions[itr, :M]
        grip = grip_config(self._sampler, self._sampler.by_share(itr))
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.vf_cem_sample_autograsp(
                self.device.index, ctypes.byref(self.cfg), ctypes.byref(grip), self.workspace.data_ptr(), int(call), int(M),
                self.elite_plans.data_ptr(), self.share.data_ptr(), out.data_ptr(), self.trials[itr].data_ptr(),
                self.capped[itr].data_ptr(), self._stream()))
        return out
