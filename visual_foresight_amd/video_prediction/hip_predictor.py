"""MI355X-native predictor with the ``VPredEvaluation`` duck-type.

Plugs into ``PixelCostController`` where the reference plugs
``robonet.video_prediction.testing.VPredEvaluation`` (reference
``visual_mpc/policy/cem_controllers/pixel_cost_controller.py:11-12,29-36,83-84,175``): ctor
``(model_path, hparams_dict, n_gpus=, first_gpu=)``, ``restore()``, ``n_context``,
``sequence_length``, ``__call__(context, {'actions'}) -> {'predicted_frames',
'predicted_pixel_distributions'}``.  Like the legacy adapter it takes the *whole* history and
slices the last ``n_context`` frames itself (reference ``video_prediction/pred_util.py:4-13``)
and chunks the sample batch by ``run_batch_size`` (``pred_util.py:21-48``; the last chunk is
simply run ragged instead of zero-padded - samples are independent).

Multi-view models (the reference's ``IndepMultiSAVP...`` family: one network per view sharing
actions and states, outputs stacked on a camera axis, ``vpred_model_interface.py:60-88``) are
one engine with ``ncam`` weight sets: every view of every sample is rolled by the same launch.

On top of that contract it offers the fused fast path ``score()``: rollouts are reduced to
per-sample costs on the GPU, sharded over the ranks of ``torch.distributed`` when that is
initialised (rank r evaluates samples ``[r*M/G, (r+1)*M/G)``; reference tower slicing
``video_prediction/setup_predictor.py:34-39``), and only the ``M`` scores are all-gathered
(RCCL) - the reference instead concatenates full predicted videos on the host
(``setup_predictor.py:155-162``).

``n_gpus`` / ``first_gpu`` mean what they mean in the reference (``setup_predictor.py:70,117-123``: ``ngpu``
towers on devices ``gpu_id ..`` inside the ONE policy process that ``sim/run.py:79-82`` creates): outside
``torch.distributed``, ``n_gpus > 1`` builds one engine per device ``first_gpu .. first_gpu + n_gpus - 1``
("lanes"), one host thread enqueues every lane's contiguous shard on its device's stream - rank-LOCAL slice
offsets, not the reference's ``gpu_id * nsmp_per_gpu`` (``setup_predictor.py:38``), which over-runs the batch
when ``first_gpu != 0`` - and the score rows are gathered with one grouped RCCL all-gather
(``vf_comm_init_all`` + ``vf_allgather_scores_group``) or, when the lanes share a device (hyper-parameter
``oversubscribe_gpus``, tests on a one-GPU box), through the host.  Under ``torch.distributed`` every rank
drives one GPU and ``n_gpus`` must be 1 or the world size.

PyTorch is the buffer carrier only: tensors own the device memory whose pointers cross the
C ABI of ``include/vf_hip.h``; all arithmetic runs in ``libvf_hip.so``.
"""
import contextlib
import ctypes
import functools
import os

import numpy as np

from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction import resample
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig, Savp2Config
from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config
from visual_foresight_amd.video_prediction.sharding import dist_info as _dist_info, shard_bounds, all_gather_rows


def transformation_of(hparams):
    """The compositing table a predictor hyper-parameter dictionary selects: ``'transformation'``: ``'cdna'`` (default),
    ``'flow'``, the appearance-flow compositing of ``cdna_arch.py``, or ``'dna'``, the per-pixel kernels of ``dna_arch.py``.
    The reference's legacy predictor configurations name it as ``'model': 'appflow'`` (``experiments/sawyer/*/conf.py``:
    "CDNA, DNA, or STP"); that key selects flow - and ``'model': 'DNA'``, in any letter case, dna - when
    ``'transformation'`` itself is absent, and every other value of ``'model'`` is left to its other readers.
    ``'transformation': 'stp'`` selects the affine warps of ``stp_arch.py``; the legacy ``'model': 'STP'`` does NOT - it keeps
    selecting ``'cdna'``, as it did before the STP table existed (``tests/test_dna.py`` pins that), so no existing
    configuration changes the network it builds."""
    legacy = {'appflow': 'flow', 'dna': 'dna'}.get(str(hparams.get('model', '')).lower(), 'cdna')
    return str(hparams.get('transformation', legacy))


def designated_pixel_count_of(hparams):
    """Designated pixels per view a predictor hyper-parameter dictionary asks for: ``'designated_pixel_count'`` (default 1).
    0 builds a FRAMES-ONLY engine - the same frames and states, no pixel distribution anywhere.  The
    reference names that mode by the bare predictor conf key ``no_pix_distrib`` (``video_prediction/setup_predictor.py:
    110-114``: ``pix_distrib = None``, ``gen_distrib`` is never built; its learned-cost experiments set it to ``''``): the
    key's presence, whatever its value, selects 0 here too."""
    if 'no_pix_distrib' in hparams:
        return 0
    n = int(hparams.get('designated_pixel_count', 1))
    if not 0 <= n <= 4:
        raise ValueError('designated_pixel_count must be 0 (frames-only) .. 4, got %r' % (n,))
    return n


def score_rows(owner, seqs, M, width, rows_of):
    """The sharded scoring driver of every cost: ``owner``'s engines roll their shares of the ``M`` actions
    whose prepared sequences are ``seqs [M * n_draws, ...]``, and the score rows are gathered -> host float64 ``[M, width]``,
    column 0 checked for the NaN of a failed rollout (``owner._check_scores``).

    ``rows_of(engine, seqs_share, n, lo)`` rolls actions ``[lo, lo + n)`` on ``engine`` and returns its device float64
    ``[n, width]`` rows; it is called under the engine's device and only enqueues work.  In-process lanes (``owner._lanes``):
    every lane's share is enqueued before anything is waited for, then one gather of the lanes' rows.  Otherwise ``owner``
    rolls its ``torch.distributed`` rank's share and the ranks all-gather (bracketed by the collective-timing events)."""
    torch, nd = owner._torch, owner.n_draws
    if getattr(owner, '_lanes', None):
        packed = []
        for lane, lo, hi in owner._lane_shares(M):
            with torch.cuda.device(lane.device):
                packed.append(rows_of(lane, seqs[lo * nd:hi * nd], hi - lo, lo) if hi > lo else
                              torch.empty((0, width), dtype=torch.float64, device=lane.device))
        rows_np = owner._gather_lane_rows(packed, M)
    else:
        rank, world = _dist_info()
        lo, hi = shard_bounds(M, rank, world)
        with torch.cuda.device(owner.device):
            rows = rows_of(owner, seqs[lo * nd:hi * nd], hi - lo, lo)
            if world > 1:
                timing = getattr(owner, '_coll_events', None)       # set_collective_timing(True): a list of events
                timed = timing is not None and len(timing) < 4096
                if timed:
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(torch.cuda.current_stream(owner.device))
                sent = rows.numel() * rows.element_size()
                rows = all_gather_rows(rows, M)
                if timed:
                    stop.record(torch.cuda.current_stream(owner.device))
                    timing.append((start, stop, sent))
            rows_np = rows.cpu().numpy()
    owner._check_scores(rows_np[:, 0])
    return rows_np


def pixel_cost_columns(rows_np, only_take_first_view):
    """Host rows ``[score | per task]`` -> (scores[M], scores_per_task[M, tasks]); ``only_take_first_view`` keeps task 0 alone
    and makes it the score (reference ``pixel_cost_controller.py:150-153``)."""
    scores_np, per_task_np = np.ascontiguousarray(rows_np[:, 0]), np.ascontiguousarray(rows_np[:, 1:])
    if only_take_first_view:
        per_task_np = per_task_np[:, :1]
        scores_np = per_task_np[:, 0].copy()
    return scores_np, per_task_np


def _scoring_entry(entry):
    """A scoring entry ``entry(self, context, inputs, ...)``: one ``_scoring_call`` around the whole call, refusals included."""
    @functools.wraps(entry)
    def scored(self, context, inputs, *args, **kwargs):
        with self._scoring_call(inputs['actions']):
            return entry(self, context, inputs, *args, **kwargs)
    return scored


class HipVPredEvaluation(object):
    wants_agent_params = True       # PixelCostController passes adim/sdim/size/sequence_length
    supports_task_weights = True    # score(..., task_weights=) applies trade-off weights on the device
    supports_frames_only = True     # designated_pixel_count 0 / no_pix_distrib: an engine without distributions
    force_frames_only = False       # FramesOnlyHipVPredEvaluation: 0 whatever the hyper-parameters say
    n_context_default = 2

    @classmethod
    def ndesig_of(cls, hparams):
        """The engine's designated-pixel count for ``hparams`` (no device needed)."""
        return 0 if cls.force_frames_only else designated_pixel_count_of(hparams)

    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        import torch
        self._torch = torch
        self._lanes = self._comms = None        # in-process multi-GPU lanes (below), their RCCL communicators
        hp = dict(hparams)
        if isinstance(model_path, (list, tuple)):
            self.model_path = [os.path.expanduser(p) for p in model_path]
        else:
            self.model_path = os.path.expanduser(model_path) if model_path else ''
        self.n_context = int(hp.get('n_context', self.n_context_default))
        self.sequence_length = int(hp.get('sequence_length', 15))
        self.n_cam = int(hp.get('ncam', 1))
        self.n_draws = int(hp.get('n_draws', 1))        # latent draws per action (stochastic_predictor.py)
        self.run_batch_size = int(hp.get('run_batch_size', 200)) * self.n_draws
        self.seed = int(hp.get('seed', 0))
        # 'arch': 'cdna' (cdna_arch.py, default), 'savp' (savp_arch.py: four scales, first-frame compositing), 'savp2'
        # (savp + the conditioning vector in every conv-LSTM + the published seven-layer compositing) or 'savp3' (savp3_arch.py:
        # the published SAVP generator; 'zdim' of the 'adim' channels are the latent, 'layer_spec' overrides the size rule)
        self.arch = str(hp.get('arch', 'cdna'))
        if self.arch not in ('cdna', 'savp', 'savp2', 'savp3'):
            raise ValueError("arch must be 'cdna', 'savp', 'savp2' or 'savp3', got %r" % (self.arch,))
        cfg_cls = {'cdna': CdnaConfig, 'savp': SavpConfig, 'savp2': Savp2Config, 'savp3': Savp3Config}[self.arch]
        extra = dict(zdim=int(hp.get('zdim', 8)), layer_spec=int(hp.get('layer_spec', 0))) if self.arch == 'savp3' else {}
        if self.arch == 'cdna' and hp.get('decoder', 'survey') != 'survey':
            extra = dict(decoder=hp['decoder'])     # 'public': the decoder widths of the public CDNA code (cdna_arch.py)
        transformation = transformation_of(hp)
        if transformation != 'cdna':
            if self.arch != 'cdna':
                raise ValueError("transformation %r needs arch 'cdna', got %r" % (transformation, self.arch))
            if transformation == 'dna':         # its own configuration class and manifest tag (dna_arch.py)
                from visual_foresight_amd.video_prediction.dna_arch import DnaConfig
                cfg_cls = DnaConfig
            elif transformation == 'stp':       # likewise (stp_arch.py)
                from visual_foresight_amd.video_prediction.stp_arch import StpConfig
                cfg_cls = StpConfig
            else:
                extra = dict(extra, transformation=transformation)
        self.cfg = cfg_cls(height=hp.get('image_height', 64), width=hp.get('image_width', 64),
                           adim=hp.get('adim', 4), sdim=hp.get('sdim', 5),
                           ndesig=self.ndesig_of(hp), n_context=self.n_context,
                           sequence_length=self.sequence_length, **extra)
        self.frames_only = self.cfg.ndesig == 0
        # 'camera_height' / 'camera_width': the context frames (and a goal picture, and what register() is given) arrive at
        # the CAMERA's resolution and are shrunk on the device to the model's (resample.py; the reference's agent does it on
        # the host, utils/im_utils.py:6-15).  None (default) = the model's size: nothing is resampled.  Everything downstream -
        # distributions, goal pixels, exported frames, render_plans - stays at the model's size.
        cam = (hp.get('camera_height'), hp.get('camera_width'))
        if (cam[0] is None) != (cam[1] is None):
            raise ValueError("'camera_height' and 'camera_width' come as a pair, got %r x %r" % cam)
        self.camera_size = None
        if cam[0] is not None and (int(cam[0]), int(cam[1])) != (self.cfg.height, self.cfg.width):
            resample.check_aspect(cam, (self.cfg.height, self.cfg.width))
            self.camera_size = (int(cam[0]), int(cam[1]))
        self._goal_cache = None         # (goal_key, the shrunk goal picture on this device) of the last keyed goal-image call
        # the image centre as goal pixels [ncam, ndesig, 2]: what the frame costs hand the rollout entry, which wants some
        self._centre_pix = np.tile(np.array([self.cfg.height // 2, self.cfg.width // 2], np.int32),
                                   (self.n_cam, self.cfg.ndesig, 1))
        if self.frames_only and self.arch == 'savp3':
            raise ValueError("arch 'savp3' has no frames-only mode (designated_pixel_count 0 / no_pix_distrib): "
                             "use 1..4 designated pixels")
        if not torch.cuda.is_available():
            raise _lib.VfError('HipVPredEvaluation needs a ROCm GPU (no CPU fallback)')
        world = _dist_info()[1]
        self.n_gpus = int(n_gpus)
        n_dev = max(torch.cuda.device_count(), 1)
        if self.n_gpus < 1:
            raise ValueError('n_gpus must be >= 1, got %r' % (n_gpus,))
        if world > 1 and self.n_gpus not in (1, world):
            raise ValueError('under torch.distributed every rank drives one GPU: n_gpus must be 1 or the world size '
                             '(%d), got %d' % (world, self.n_gpus))
        oversubscribe = bool(int(hp.get('oversubscribe_gpus', os.environ.get('VF_OVERSUBSCRIBE_GPUS', 0))))
        if world == 1 and self.n_gpus > n_dev and not oversubscribe:
            raise ValueError('n_gpus=%d but this host exposes %d GPU(s) (set the predictor hyper-parameter '
                             "'oversubscribe_gpus' to let the lanes share devices)" % (self.n_gpus, n_dev))
        if world == 1 and not oversubscribe and (int(first_gpu) < 0 or int(first_gpu) + self.n_gpus > n_dev):
            # devices first_gpu .. first_gpu + n_gpus - 1 are promised: never wrap onto GPUs below first_gpu,
            # which another policy process may own (reference sim/run.py hands out disjoint gpu_id ranges)
            raise ValueError('first_gpu=%d + n_gpus=%d exceeds the %d GPU(s) of this host (set the predictor '
                             "hyper-parameter 'oversubscribe_gpus' to wrap around)"
                             % (int(first_gpu), self.n_gpus, n_dev))
        # under torchrun LOCAL_RANK picks this rank's GPU; the lanes of the in-process mode follow first_gpu
        local_rank = int(os.environ.get('LOCAL_RANK', 0)) if world > 1 else 0
        shared_dry_run = oversubscribe or os.environ.get('VF_BENCH_BACKEND') == 'gloo'
        if world > 1 and not shared_dry_run and (int(first_gpu) < 0 or int(first_gpu) + local_rank >= n_dev):
            import torch.distributed as dist
            if dist.get_backend() != 'gloo':
                # one process per GPU: rank r owns device first_gpu + LOCAL_RANK - never wrap onto a GPU below first_gpu
                # (another job's), and never put two RCCL ranks on one device
                raise ValueError('first_gpu=%d + LOCAL_RANK=%d is outside the %d GPU(s) of this host (ranks sharing a '
                                 "GPU need the gloo backend or the hyper-parameter 'oversubscribe_gpus')"
                                 % (int(first_gpu), local_rank, n_dev))
        self.device_index = (int(first_gpu) + local_rank) % n_dev
        self.device = torch.device('cuda', self.device_index)
        self._libh = _lib.load_library()
        c = self.cfg
        # 'fp32' (default): exact fp32 MFMA.  'bf16x6': fp32 emulated by six bf16 MFMA products in the
        # conv-LSTM gate GEMMs (fp32-class accuracy, not bit-identical to 'fp32').
        # The reference's reduced-precision switch is the bare key 'float16' in the predictor conf
        # (video_prediction/setup_predictor.py:92-95: placeholders and model in tf.float16).  Its counterpart here is
        # the split-bf16 mode: the same kind of opt-in for speed, but with fp32-class accuracy.
        # 'bf16' (2): plain bf16 - operands of the gate GEMMs rounded once, one bf16 MFMA product per multiply, fp32
        # accumulation.  THIS is the mode with the reference's speed / accuracy trade (half-precision arithmetic for
        # speed); the bare 'float16' key keeps selecting 'bf16x6', so ask for it by name: precision='bf16' or
        # VF_PRECISION=bf16.
        default_precision = 'bf16x6' if 'float16' in hp else os.environ.get('VF_PRECISION', 'fp32')
        precision = hp.get('precision', default_precision)
        self.precision = {'fp32': 0, '0': 0, 0: 0, 'bf16x6': 1, '1': 1, 1: 1, 'bf16': 2, '2': 2, 2: 2}[precision]
        self._c_cfg = _lib.VfConfig(c.height, c.width, c.adim, c.sdim, c.ndesig, c.n_context,
                                    c.sequence_length, c.num_masks, self.run_batch_size,
                                    self.device_index, self.precision, self.n_cam, self.n_draws, c.arch_id,
                                    getattr(c, 'zdim', 0), getattr(c, 'layer_spec', 0))
        self._handle = ctypes.c_void_p()
        _lib.check(self._libh.vf_create(ctypes.byref(self._c_cfg), ctypes.byref(self._handle)))
        self.set_dedup(int(hp.get('dedup', os.environ.get('VF_DEDUP', 1))))
        self.set_persistent(int(hp.get('persistent', os.environ.get('VF_PERSISTENT', 1))))
        self.set_xcd_queues(int(hp.get('xcd_queues', os.environ.get('VF_XCD_QUEUES', 1))))
        self.set_fuse_top(int(hp.get('fuse_top', os.environ.get('VF_FUSE_TOP', 1))))
        self.weights = None
        self._ctx_key = None
        self._last_M = 0
        self._last_lo = 0
        self._last_prepared = None      # (engine context, sequences, M) of the last score() / __call__
        self.last_goal_cost_per_step = None     # [M, ncam, T] of the last score_goal_image()
        self.last_frame_cost_per_step = None    # [M, T] of the last score_frames()
        self._lane_scorers = {}                 # id(scorer) -> (scorer, its copy on this lane's device); one entry per scorer seen
        # in-process multi-GPU: this object is lane 0, the others are plain engines on the following devices
        self.gather = str(hp.get('gather', 'auto'))         # 'auto' | 'rccl' | 'host'
        if self.gather not in ('auto', 'rccl', 'host'):
            raise ValueError("gather must be 'auto', 'rccl' or 'host'")
        if world == 1 and self.n_gpus > 1 and not hp.get('_lane'):
            lane_hp = dict(hp, _lane=True, oversubscribe_gpus=1)
            lane_hp['designated_pixel_count'] = self.cfg.ndesig     # (a frames-only predictor's lanes are frames-only)
            lane_hp.pop('no_pix_distrib', None)
            self._lanes = [self] + [HipVPredEvaluation(model_path, lane_hp, n_gpus=1, first_gpu=int(first_gpu) + i)
                                    for i in range(1, self.n_gpus)]
            distinct = len({l.device_index for l in self._lanes}) == self.n_gpus
            if self.gather == 'rccl' and not distinct:
                raise ValueError("gather='rccl' needs one distinct GPU per lane")
            self._use_rccl = distinct if self.gather == 'auto' else self.gather == 'rccl'

    def _all_lanes(self):
        return self._lanes if self._lanes else [self]

    def __del__(self):
        try:
            for comm in (getattr(self, '_comms', None) or []):
                self._libh.vf_comm_destroy(comm)
            self._comms = None
            if getattr(self, '_handle', None) and self._handle.value:
                self._libh.vf_destroy(self._handle)
                self._handle = ctypes.c_void_p()
        except Exception:   # interpreter shutdown
            pass

    # ------------------------------------------------------------------ measurement hooks
    def set_profiling(self, enable):
        _lib.check(self._libh.vf_set_profiling(self._handle, int(bool(enable))))

    def get_profile(self):
        """-> (kernel_ms, launches, flops, busy_ms) of the conv-LSTM kernel since the last call."""
        ms, n, fl, busy = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.check(self._libh.vf_get_profile(self._handle, ctypes.byref(ms), ctypes.byref(n),
                                             ctypes.byref(fl), ctypes.byref(busy)))
        return ms.value, n.value, fl.value, busy.value

    def _set_on_lanes(self, entry, *args, **attributes):
        """``entry(handle, *args)`` of the library on every lane, under its device; ``attributes`` record the setting on it."""
        for lane in self._all_lanes():
            with self._torch.cuda.device(lane.device):
                _lib.check(getattr(lane._libh, entry)(lane._handle, *args))
            for name, value in attributes.items():
                setattr(lane, name, value)

    def set_persistent(self, enable):
        """Run each rollout as one persistent launch (bit-identical results; see vf_persistent.h)."""
        self._set_on_lanes('vf_set_persistent', int(bool(enable)), persistent=bool(enable))

    def set_xcd_queues(self, enable):
        """One ticket queue per XCD (default) or plain phase order; placement only, bit-identical results."""
        self._set_on_lanes('vf_set_xcd_queues', int(bool(enable)), xcd_queues=bool(enable))

    def set_fuse_top(self, enable):
        """Top transposed conv + compositing as one item per tile (vf_set_fuse_top); bit-identical results."""
        self._set_on_lanes('vf_set_fuse_top', int(bool(enable)), fuse_top=bool(enable))

    def set_sched_option(self, option, value):
        """Timing-only options of the persistent launch (``vf_set_sched_option``): ``'yield_budget'`` (0 = off, -1 = automatic)
        and ``'write_through'`` (0 / 1).  Results are bit-identical for every setting."""
        self._set_on_lanes('vf_set_sched_option', {'yield_budget': 0, 'write_through': 1}[option], int(value))

    def device_status(self):
        """Synchronise, return the sticky failure word of the persistent kernel (0 = healthy), re-arm it."""
        worst = 0
        for lane in self._all_lanes():
            st = ctypes.c_int32()
            with self._torch.cuda.device(lane.device):
                _lib.check(lane._libh.vf_device_status(lane._handle, ctypes.byref(st)))
            worst = max(worst, st.value)
        return worst

    def _check_scores(self, scores_np):
        """A rollout whose tiles gave up waiting poisons its scores with NaN (vf_hip.h): never hand
        them to the elite selection."""
        if np.isnan(scores_np).any():
            for lane in self._all_lanes():      # the engine drops its context-only cache with the status:
                lane._ctx_key = None            # upload the context again
            raise _lib.VfError('the persistent rollout kernel reported a failure (device status %d): a tile gave '
                               'up waiting for its producers; scores are invalid' % self.device_status())

    def _check_status(self):
        """The same refusal for a frames-only rollout, which has no pixel scores to poison: read the failure word."""
        st = self.device_status()
        if st != 0:
            for lane in self._all_lanes():
                lane._ctx_key = None
            raise _lib.VfError('the persistent rollout kernel reported a failure (device status %d): a tile gave '
                               'up waiting for its producers; predictions are invalid' % st)

    def set_dedup(self, enable):
        """Switch context de-duplication (bit-identical results either way; for A/B timing)."""
        self._set_on_lanes('vf_set_dedup', int(bool(enable)))

    # ------------------------------------------------------------------ weights
    def restore(self, weights=None):
        """Load ``model_path`` (manifest.json + weights.bin; ``view%d/`` sub-directories or a list of paths for
        several views) or, with no path, seeded random weights (seed + view)."""
        if weights is None:
            weights = []
            for v in range(self.n_cam):
                path = self.model_path[v] if isinstance(self.model_path, (list, tuple)) else self.model_path
                if path and self.n_cam > 1 and os.path.isdir(os.path.join(path, 'view%d' % v)):
                    path = os.path.join(path, 'view%d' % v)
                weights.append(CdnaWeights.load(path, self.cfg) if path else
                               CdnaWeights.random(self.cfg, seed=self.seed + v))
        elif not isinstance(weights, (list, tuple)):
            weights = [weights]
        if len(weights) != self.n_cam:
            raise ValueError('need one weight set per view (%d), got %d' % (self.n_cam, len(weights)))
        self.weights = weights[0] if self.n_cam == 1 else list(weights)
        self._ctx_key = None
        blob = np.concatenate([v.ravel() for w in weights for v in w.tensors.values()]).astype(np.float32)
        want = self._libh.vf_weight_count(ctypes.byref(self._c_cfg)) * self.n_cam
        if blob.size != want:
            raise _lib.VfError('weight blob has %d floats, library expects %d' % (blob.size, want))
        with self._torch.cuda.device(self.device):      # the library selects the engine's device: put the caller's back
            _lib.check(self._libh.vf_load_weights(self._handle, blob.ctypes.data_as(ctypes.c_void_p),
                                                  blob.size))
        for lane in (self._lanes or [])[1:]:        # the weights are replicated on every lane's device
            lane.restore(list(weights))
        return self

    # ------------------------------------------------------------------ context
    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _set_context(self, context):
        torch, c = self._torch, self.cfg
        frames, states, acts, distrib = self._context_arrays(context)
        # the CEM iterations of one planning call pass the same context: upload it (and let the
        # engine recompute the context-only part of the network) only when it actually changed
        key = (frames, states, acts, distrib)
        if self._ctx_key is not None and all(np.array_equal(a, b) for a, b in zip(key, self._ctx_key)):
            return
        self._ctx_key = tuple(a.copy() for a in key)
        dev = self.device
        self._ctx = [torch.from_numpy(a).to(dev) for a in (frames, states, acts, distrib)]
        if self.camera_size is not None:        # uploaded once at the camera's size, shrunk into the buffer the engine reads
            with torch.cuda.device(dev):
                self._ctx[0] = resample.area_resize_device(self._ctx[0], (c.height, c.width))
        f, s, a, d = self._ctx
        _lib.check(self._libh.vf_set_context(self._handle, f.data_ptr(), s.data_ptr(), a.data_ptr(),
                                             None if self.frames_only else d.data_ptr(), self._stream()))

    # ------------------------------------------------------------------ rollouts
    def _rollout_chunk(self, actions_dev, goal_pix, finalweight, scores_dev, per_task_dev, task_weights=None):
        B = actions_dev.shape[0]
        if self.frames_only:        # no goal pixel, no pixel cost: the library wants NULL for all of them
            _lib.check(self._libh.vf_rollout(self._handle, actions_dev.data_ptr(), B, None, ctypes.c_float(finalweight),
                                             None, None, None, self._stream()))
            return
        ntask = self.n_cam * self.cfg.ndesig
        goal = np.asarray(goal_pix).reshape(-1)
        if goal.size != 2 * ntask:
            raise ValueError('goal_pix must hold [ncam=%d][ndesig=%d][2] values, got %d'
                             % (self.n_cam, self.cfg.ndesig, goal.size))
        goal_c = (ctypes.c_int32 * (2 * ntask))(*[int(v) for v in goal])
        _lib.check(self._libh.vf_rollout(self._handle, actions_dev.data_ptr(), B, goal_c,
                                         ctypes.c_float(finalweight), self._task_weights_c(task_weights),
                                         scores_dev.data_ptr(), per_task_dev.data_ptr(), self._stream()))

    def _task_weights_c(self, task_weights):
        """``task_weights`` ([ncam, ndesig], or None for the plain mean over tasks) as the library takes them."""
        if task_weights is None:
            return None
        ntask = self.n_cam * self.cfg.ndesig
        w = np.asarray(task_weights, dtype=np.float64).reshape(-1)
        if w.size != ntask:
            raise ValueError('task_weights must hold ncam*ndesig = %d values' % ntask)
        return (ctypes.c_float * ntask)(*[float(v) for v in w])

    def _check_actions(self, actions):
        actions = np.asarray(actions)
        T = self.sequence_length - self.n_context
        if actions.ndim != 3 or actions.shape[1] != T or actions.shape[2] != self._adim_in():
            raise ValueError('actions must be [M, %d, %d], got %s' % (T, self._adim_in(), actions.shape))
        return actions

    # hooks of the stochastic predictor: the caller's actions -> the sequences the engine rolls
    def _adim_in(self):
        return self.cfg.adim

    def _prepare(self, context, actions):
        """(context, actions[n]) -> (engine context, sequences[n * n_draws])."""
        return context, actions

    def _prepare_device(self, context, actions_dev):
        """``_prepare`` for candidates that lie on this engine's device (the ``score*_device`` entries; only enqueues, under
        this engine's device): nothing here.  A class that overrides ``_prepare`` brings its own or refuses the device entries
        (``_prepares_on_host``)."""
        return context, actions_dev

    def _prepares_on_host(self):
        """Whether the device entries cannot serve this class: its ``_prepare`` is overridden below the ``_prepare_device`` it
        would run with (that hook prepares something else), or several draws per action meet the plain hook."""
        mro = type(self).__mro__
        host, device = (next(i for i, c in enumerate(mro) if name in vars(c)) for name in ('_prepare', '_prepare_device'))
        return device > host or (type(self)._prepare_device is HipVPredEvaluation._prepare_device and self.n_draws != 1)

    def _scoring_call(self, actions):
        """Context manager around one scoring call on ``actions`` (``score*``; the ensemble enters member 0's): nothing here,
        the stochastic predictor holds the call's latent draws in it."""
        return contextlib.nullcontext()

    def _lane_shares(self, M):
        """(lane, lo, hi): every lane's contiguous share ``[lo, hi)`` of ``M`` actions, in lane order.  A lane whose share is
        empty holds nothing of this call: its resident range is emptied, so that a stale one cannot match a fetch."""
        for i, lane in enumerate(self._lanes):
            lo, hi = shard_bounds(M, i, len(self._lanes))
            if hi == lo:
                lane._last_lo, lane._last_M = lo, 0
            yield lane, lo, hi

    def _score_prepared(self, context, seqs, n, goal_pix, finalweight, index_base=0, task_weights=None,
                        after_chunk=None):
        """Roll ``seqs [n * n_draws, T, engine adim]`` (as ``_prepare`` returns them) on this engine -> device tensors
        (scores[n], per_task[n, ncam*nd]).  ``index_base`` is the global index of the first action (what
        ``fetch_pixel_distributions`` is asked for).  Only enqueues work on this engine's device (the uploads of
        pageable host arrays aside).  ``after_chunk(c0, c1)`` runs after the rollout of actions ``[c0, c1)``, while
        their predictions are resident (``score_goal_image`` reduces them there)."""
        torch = self._torch
        ntask = self.n_cam * self.cfg.ndesig
        nd = self.n_draws
        self._set_context(context)
        if torch.is_tensor(seqs):       # score_device: the sequences already lie on this device
            local = seqs
        else:
            local = torch.from_numpy(np.ascontiguousarray(seqs, dtype=np.float32)).to(self.device)
        scores = torch.empty(n, dtype=torch.float64, device=self.device)
        per_task = torch.empty((n, ntask), dtype=torch.float64, device=self.device)
        bs = self.run_batch_size // nd          # actions per chunk
        for c0 in range(0, n, bs):
            c1 = min(c0 + bs, n)
            self._rollout_chunk(local[c0 * nd:c1 * nd], goal_pix, finalweight, scores[c0:c1], per_task[c0:c1],
                                task_weights)
            self._last_lo, self._last_M = index_base + c0, c1 - c0
            if after_chunk is not None:
                after_chunk(c0, c1)
        return scores, per_task

    def _roll_and_reduce(self, context, seqs, n, index_base, widths, reduce):
        """Roll ``n`` actions on this engine (the image centre as goal pixels, their pixel scores dropped) and reduce every
        chunk while its frames are resident: ``reduce(*scratch)`` makes the one library call that fills the scratch tensors
        ``[chunk, w]``, one per column group ``w`` of ``widths`` -> device rows ``[n, sum(widths)]``."""
        torch = self._torch
        bs = self.run_batch_size // self.n_draws
        rows = torch.empty((n, sum(widths)), dtype=torch.float64, device=self.device)
        scratch = [torch.empty((bs, w), dtype=torch.float64, device=self.device) for w in widths]

        def reduce_chunk(c0, c1):
            reduce(*scratch)
            col = 0
            for s, w in zip(scratch, widths):
                rows[c0:c1, col:col + w] = s[:c1 - c0]
                col += w

        self._score_prepared(context, seqs, n, self._centre_pix, 1.0, index_base=index_base, after_chunk=reduce_chunk)
        return rows

    @_scoring_entry
    def score(self, context, inputs, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
        """Fused rollout + expected-pixel-distance cost.  Returns (scores[M], scores_per_task[M, ncam*nd]) float64.

        ``task_weights`` ([ncam, ndesig] trade-off weights, reference ``register_gtruth_controller.py:88-94``)
        replace the plain mean over tasks.  Only the chunk evaluated last stays resident for
        ``fetch_pixel_distributions``; with ``M <= run_batch_size`` (the reference default,
        ``pixel_cost_controller.py:31``) that is the whole local shard.
        """
        self._refuse_frames_only('score')
        actions = self._check_actions(inputs['actions'])
        M = actions.shape[0]
        # every rank / lane slices the SAME prepared sequences (latent draws included); they are also what a
        # propagation fetch of a sample that is no longer resident is re-rolled from
        ctx_p, seqs = self._prepare(context, actions)
        self._last_prepared = (ctx_p, seqs, M)

        def rows_of(lane, share, n, lo):        # [score | per task]
            s, pt = lane._score_prepared(ctx_p, share, n, goal_pix, finalweight, index_base=lo, task_weights=task_weights)
            return self._torch.cat([s[:, None], pt], dim=1)

        rows_np = score_rows(self, seqs, M, 1 + self.n_cam * self.cfg.ndesig, rows_of)
        return pixel_cost_columns(rows_np, only_take_first_view)

    # ------------------------------------------------------------------ batched planning: G problems in one rollout
    def _context_arrays(self, context):
        """One context dictionary -> the arrays the engine is given: (frames, states, actions, distributions), the last
        ``n_context`` steps, checked (frames at the model's or - ``camera_size`` - the camera's size).  The one source of
        ``_set_context`` and ``_set_contexts``."""
        nc, c = self.n_context, self.cfg
        ncam = self.n_cam
        frames = np.ascontiguousarray(np.asarray(context['context_frames'])[-nc:, :ncam])
        if self.camera_size is not None:
            if frames.dtype != np.uint8 or frames.shape != (nc, ncam) + self.camera_size + (3,):
                raise ValueError('context_frames must be uint8 [>=%d, %d, %d, %d, 3] at the camera size %d x %d (the model '
                                 'size is %d x %d: they are shrunk on the device), got %s %s'
                                 % ((nc, ncam) + self.camera_size + self.camera_size + (c.height, c.width, frames.dtype,
                                                                                       frames.shape)))
        elif frames.dtype != np.uint8 or frames.shape != (nc, ncam, c.height, c.width, 3):
            raise ValueError('context_frames must be uint8 [>=%d, %d, %d, %d, 3], got %s %s'
                             % (nc, ncam, c.height, c.width, frames.dtype, frames.shape))
        if self.frames_only:
            if context.get('context_pixel_distributions') is not None:
                raise ValueError('this predictor is frames-only (designated_pixel_count 0 / no_pix_distrib): the context '
                                 'must not carry context_pixel_distributions')
            distrib = np.zeros((nc, ncam, c.height, c.width, 0), np.float32)
        else:
            distrib = np.ascontiguousarray(
                np.asarray(context['context_pixel_distributions'], dtype=np.float32)[-nc:, :ncam])
        states = np.ascontiguousarray(np.asarray(context['context_states'], dtype=np.float32)[-nc:])
        if states.shape != (nc, c.sdim) or distrib.shape != (nc, ncam, c.height, c.width, c.ndesig):
            raise ValueError('bad context shapes: states %s distrib %s' % (states.shape, distrib.shape))
        if nc > 1:
            acts = np.asarray(context['context_actions'], dtype=np.float32).reshape(-1, c.adim)[-(nc - 1):]
            if acts.shape[0] != nc - 1:
                raise ValueError('need at least %d executed actions as context' % (nc - 1))
            acts = np.ascontiguousarray(acts)
        else:
            acts = np.zeros((1, c.adim), np.float32)
        return frames, states, acts, distrib

    def grouped_refusal(self):
        """Why this predictor cannot roll grouped contexts (``_set_contexts``), or None when it can."""
        if self._lanes:
            return 'grouped contexts drive one engine: this predictor has %d in-process lanes (n_gpus > 1)' % len(self._lanes)
        if _dist_info()[1] > 1:
            return 'grouped contexts drive one engine: torch.distributed has %d ranks' % _dist_info()[1]
        if self.n_draws != 1:
            return 'grouped contexts need n_draws = 1, this predictor has %d' % self.n_draws
        if type(self)._prepare is not HipVPredEvaluation._prepare:
            return 'grouped contexts roll the actions as they are given: %s overrides _prepare' % type(self).__name__
        if self.arch != 'cdna':
            return "grouped contexts need arch 'cdna', this predictor has %r" % (self.arch,)
        return None

    def score_batch_refusal(self):
        """Why ``score_batch`` cannot serve this predictor, or None when it can: ``grouped_refusal``'s reasons, and a
        frames-only engine (it may still roll grouped contexts; only the pixel cost is refused)."""
        reason = self.grouped_refusal()
        if reason is None and self.frames_only:
            reason = ('score_batch needs pixel distributions; this predictor is frames-only (designated_pixel_count 0 / '
                      'no_pix_distrib)')
        return reason

    def _set_contexts(self, contexts, rows_per_group):
        """Upload ``contexts`` (a list of G context dictionaries) as the grouped contexts of the coming rollout of
        ``G * rows_per_group`` rows: one ``vf_set_contexts``.  The single-context key is dropped - the next single-context call
        uploads its context again."""
        reason = self.grouped_refusal()
        if reason:
            raise ValueError(reason)
        torch, c = self._torch, self.cfg
        G = len(contexts)
        if G < 1 or rows_per_group < 1 or G * rows_per_group > self.run_batch_size:
            raise ValueError('grouped contexts: %d problems x %d rows do not fit run_batch_size = %d (all rows of a call '
                             'stay resident in one chunk)' % (G, rows_per_group, self.run_batch_size))
        parts = [self._context_arrays(ctx) for ctx in contexts]
        frames, states, acts, distrib = (np.stack([p[i] for p in parts]) for i in range(4))
        self._ctx_key = None
        dev = self.device
        with torch.cuda.device(dev):
            f, s, a, d = self._ctx = [torch.from_numpy(x).to(dev) for x in (frames, states, acts, distrib)]
            if self.camera_size is not None:    # [G, nc, ncam] images at the camera's size, shrunk where the engine reads them
                f = self._ctx[0] = resample.area_resize_device(f, (c.height, c.width))
            _lib.check(self._libh.vf_set_contexts(self._handle, G, int(rows_per_group), f.data_ptr(), s.data_ptr(),
                                                  a.data_ptr(), None if self.frames_only else d.data_ptr(), self._stream()))

    def score_batch(self, contexts, inputs, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
        """``score`` for G independent planning problems in ONE rollout launch.  ``contexts``: a list of G context
        dictionaries, each what ``score`` takes; ``inputs['actions']`` ``[G, M, T, adim]``; ``goal_pix`` ``[G, ncam, ndesig,
        2]``; ``task_weights`` ``[G, ncam, ndesig]`` or None -> float64 ``(scores [G, M], scores_per_task [G, M, tasks])``.
        One ``vf_set_contexts``, one ``vf_rollout``, one ``vf_group_pixel_scores``; ``G * M <= run_batch_size``, so all rows
        stay resident: ``fetch_pixel_distributions(g * M + i)`` returns row ``i`` of problem ``g``.  ValueError: see
        ``score_batch_refusal``."""
        reason = self.score_batch_refusal()
        if reason:
            raise ValueError(reason)
        torch = self._torch
        actions = np.asarray(inputs['actions'])
        G = len(contexts)
        T = self.sequence_length - self.n_context
        if actions.ndim != 4 or actions.shape[0] != G or actions.shape[2:] != (T, self.cfg.adim) or actions.shape[1] < 1:
            raise ValueError('actions must be [G=%d, M, %d, %d], got %s' % (G, T, self.cfg.adim, actions.shape))
        M = actions.shape[1]
        ntask = self.n_cam * self.cfg.ndesig
        goal = np.ascontiguousarray(np.asarray(goal_pix).reshape(-1).astype(np.int32))
        if goal.size != G * ntask * 2:
            raise ValueError('goal_pix must hold [G=%d][ncam=%d][ndesig=%d][2] values, got %d'
                             % (G, self.n_cam, self.cfg.ndesig, goal.size))
        weights_c = None
        if task_weights is not None:
            w = np.asarray(task_weights, dtype=np.float64).reshape(-1)
            if w.size != G * ntask:
                raise ValueError('task_weights must hold G * ncam * ndesig = %d values' % (G * ntask))
            weights_c = (ctypes.c_float * (G * ntask))(*[float(v) for v in w])
        self._set_contexts(contexts, M)
        with torch.cuda.device(self.device):
            seqs = torch.from_numpy(np.ascontiguousarray(actions.reshape(G * M, T, -1), dtype=np.float32)).to(self.device)
            goal_dev = torch.from_numpy(goal).to(self.device)
            scores, per_task = (torch.empty(s, dtype=torch.float64, device=self.device) for s in ((G * M,), (G * M, ntask)))
            # (vf_rollout's own scores - every row against problem 0's goal - are overwritten by the grouped cost)
            self._rollout_chunk(seqs, goal[:2 * ntask], finalweight, scores, per_task)
            _lib.check(self._libh.vf_group_pixel_scores(self._handle, goal_dev.data_ptr(), ctypes.c_float(finalweight),
                                                        weights_c, scores.data_ptr(), per_task.data_ptr(), self._stream()))
            rows_np = torch.cat([scores[:, None], per_task], dim=1).cpu().numpy()
        # what is resident: rows [0, G * M) of this call; a fetch of anything else has nothing to re-roll from
        self._last_lo, self._last_M = 0, G * M
        self._last_prepared = None
        self._check_scores(rows_np[:, 0])
        scores_np, per_task_np = pixel_cost_columns(rows_np, only_take_first_view)
        return scores_np.reshape(G, M), per_task_np.reshape(G, M, -1)

    def score_device_refusal(self):
        """Why ``score_device`` cannot serve this predictor, or None when it can (a planner asks before it commits a planning
        call to the device route)."""
        if self.frames_only:
            return ('score_device needs pixel distributions; this predictor is frames-only (designated_pixel_count 0 / '
                    'no_pix_distrib)')
        if self._lanes:
            return 'score_device drives one engine: this predictor has %d in-process lanes (n_gpus > 1)' % len(self._lanes)
        if _dist_info()[1] > 1:
            return 'score_device drives one engine: torch.distributed has %d ranks' % _dist_info()[1]
        if self._prepares_on_host():
            return 'score_device rolls the actions as they lie on the device: %s prepares its sequences on the host' \
                   % type(self).__name__
        return None

    def score_device(self, context, actions_dev, goal_pix, finalweight=10., only_take_first_view=False, task_weights=None):
        """``score`` without the gather: roll ``actions_dev`` - a contiguous float32 tensor ``[M, T, adim]`` on this engine's
        device - and return the device float64 ``scores [M]``.  Only enqueues (the context upload aside, when it changed);
        the caller checks the downloaded scores with ``_check_scores``.  Chunked by ``run_batch_size`` like ``score``; the last
        chunk stays resident for ``render_plans`` / ``fetch_pixel_distributions``, and ``actions_dev`` must stay untouched for
        as long as those may be asked for.  The per-task scores of the call are kept in ``last_per_task_dev`` ``[M, tasks]``.
        ValueError: lanes, a ``torch.distributed`` world, sequences prepared on the host, a frames-only engine."""
        reason = self.score_device_refusal()
        if reason:
            raise ValueError(reason)
        torch = self._torch
        M = self._check_actions_dev(actions_dev)
        with torch.cuda.device(self.device):
            ctx_p, seqs = self._prepare_device(context, actions_dev)
            self._last_prepared = (ctx_p, seqs, M)
            scores, per_task = self._score_prepared(ctx_p, seqs, M, goal_pix, finalweight, index_base=0,
                                                    task_weights=task_weights)
            if only_take_first_view:        # task 0 alone is the score (pixel_cost_columns)
                per_task = per_task[:, :1]
                scores = per_task[:, 0].contiguous()
        self.last_per_task_dev = per_task
        return scores

    def _check_actions_dev(self, actions_dev):
        """The candidates of a ``score*_device`` entry: a contiguous float32 tensor ``[M, T, adim]`` on this engine's device
        -> ``M``."""
        torch = self._torch
        T = self.sequence_length - self.n_context
        if not torch.is_tensor(actions_dev) or actions_dev.device != self.device or actions_dev.dtype != torch.float32 \
                or not actions_dev.is_contiguous() or tuple(actions_dev.shape[1:]) != (T, self._adim_in()) \
                or actions_dev.shape[0] < 1:
            raise ValueError('actions_dev must be a contiguous float32 tensor [M, %d, %d] on %s'
                             % (T, self._adim_in(), self.device))
        return int(actions_dev.shape[0])

    def frame_score_device_refusal(self):
        """Why ``score_goal_image_device`` / ``score_frames_device`` cannot serve this predictor, or None when they can: every
        clause of ``score_device_refusal`` but the frames-only one - a frame cost needs no distribution."""
        if self._lanes:
            return 'the device entries drive one engine: this predictor has %d in-process lanes (n_gpus > 1)' % len(self._lanes)
        if _dist_info()[1] > 1:
            return 'the device entries drive one engine: torch.distributed has %d ranks' % _dist_info()[1]
        if self._prepares_on_host():
            return 'the device entries roll the actions as they lie on the device: %s prepares its sequences on the host' \
                   % type(self).__name__
        return None

    def _refuse_frames_only(self, what):
        if self.frames_only:
            raise ValueError('%s needs pixel distributions; this predictor is frames-only (designated_pixel_count 0 / '
                             'no_pix_distrib)' % what)

    def _centre_context(self, context):
        """``context`` as the frame costs roll it: with the image centre switched on in the distribution channels the
        network carries - or, frames-only, as it is (there is no such channel)."""
        if self.frames_only:
            return context
        c = self.cfg
        centre = np.zeros((self.n_context, self.n_cam, c.height, c.width, c.ndesig), np.float32)
        centre[:, :, c.height // 2, c.width // 2, :] = 1.0
        return dict(context, context_pixel_distributions=centre)

    # ------------------------------------------------------------------ goal-image cost
    def _check_goal_image(self, goal_image):
        """-> float32 ``[ncam, H, W, 3]``: uint8 is scaled by 1/255 as ``get_context`` scales context frames (reference
        ``video_prediction/pred_util.py:4-13``), floating point is taken as it is."""
        c = self.cfg
        g = np.asarray(goal_image)
        if g.ndim == 3 and self.n_cam == 1:
            g = g[None]
        sizes = [(c.height, c.width)] + ([self.camera_size] if self.camera_size is not None else [])
        if g.shape not in [(self.n_cam,) + sz + (3,) for sz in sizes]:
            raise ValueError('goal_image must be [%d, %s, 3]%s, got %s'
                             % (self.n_cam, ' or '.join('%d, %d' % sz for sz in sizes),
                                ' or [H, W, 3]' if self.n_cam == 1 else '', g.shape))
        if g.dtype == np.uint8:
            return np.ascontiguousarray(g.astype(np.float32) / np.float32(255.))
        if not np.issubdtype(g.dtype, np.floating):
            raise ValueError('goal_image must be uint8 or floating point, got %s' % g.dtype)
        return np.ascontiguousarray(g, dtype=np.float32)

    def _goal_on_device(self, goal, goal_key=None):
        """``goal`` (float32, from ``_check_goal_image``) on this engine's device at the model's size.  A goal picture at the
        camera's size is shrunk there with the float32 path of ``vf_resize_area`` (reference ``goal_im_controller.py:89``).
        ``goal_key``: the caller's name for this picture (``GoalImController`` counts its ``act()`` calls); a call with the key
        of the previous one finds the shrunk copy - no upload, no launch, and the pictures are never compared.  Without a
        key the picture is uploaded and shrunk in every call."""
        torch, c = self._torch, self.cfg
        if goal.shape[1:3] == (c.height, c.width):
            return torch.from_numpy(goal).to(self.device)
        if goal_key is not None and self._goal_cache is not None and self._goal_cache[0] == goal_key:
            return self._goal_cache[1]
        with torch.cuda.device(self.device):
            small = resample.area_resize_device(torch.from_numpy(goal).to(self.device), (c.height, c.width))
        self._goal_cache = None if goal_key is None else (goal_key, small)
        return small

    @_scoring_entry
    def score_goal_image(self, context, inputs, goal_image, steps='last', finalweight=10., first_view_only=False,
                         goal_key=None):
        """Fused rollout + goal-image cost (reference ``policy/cem_controllers/goal_im_controller.py:93``): the mean
        squared error between predicted frames and ``goal_image``, reduced on the GPU from the frames resident in the
        engine.  Returns (scores[M], scores_per_view[M, ncam]) float64; ``last_goal_cost_per_step`` ``[M, ncam, T]``
        keeps the per-step MSE (averaged over latent draws).

        ``goal_image``: ``[ncam, H, W, 3]`` (or ``[H, W, 3]`` with one view); uint8 is scaled by 1/255 like the
        context frames, floating point is compared as it is.  With ``camera_height`` / ``camera_width`` it may also come at
        the camera's size: it is then shrunk on the device (after the scaling, in float32) - in every call, or, with a
        ``goal_key`` (any hashable the caller changes with the picture), once per key.
        ``steps='last'`` scores the last predicted frame, ``'weighted'`` the time-weighted mean with ``w = (1, ..., 1, finalweight)``.  ``first_view_only`` takes view 0's
        cost as the score instead of the mean over views (``scores_per_view`` keeps every view).

        Sharding, chunking, lanes and latent draws are those of ``score``.  The rollout entry still wants goal pixels
        and a distribution context: the image centre is passed for both (``context_pixel_distributions`` of
        ``context`` is not read) and its pixel scores are dropped - the price is the ``ndesig`` distribution
        channels the network carries anyway.  A frames-only predictor carries none and passes neither."""
        goal, mode = self._check_goal_cost(goal_image, steps)
        actions = self._check_actions(inputs['actions'])
        M = actions.shape[0]
        ncam, T = self.n_cam, self.sequence_length - self.n_context
        ctx_p, seqs = self._prepare(self._centre_context(context), actions)
        self._last_prepared = (ctx_p, seqs, M)

        def rows_of(lane, share, n, lo):
            return lane._goal_rows(ctx_p, share, n, lo, goal, goal_key, mode, finalweight, first_view_only)

        rows_np = score_rows(self, seqs, M, 1 + ncam + ncam * T, rows_of)
        scores, per_view, self.last_goal_cost_per_step = self.split_goal_rows(rows_np)
        return scores, per_view

    def _check_goal_cost(self, goal_image, steps):
        """The argument checks of the goal-image entries -> (float32 goal, the kernel's mode)."""
        goal = self._check_goal_image(goal_image)
        if steps not in ('last', 'weighted'):
            raise ValueError("steps must be 'last' or 'weighted', got %r" % (steps,))
        return goal, 1 if steps == 'weighted' else 0

    def _goal_rows(self, ctx_p, seqs, n, lo, goal, goal_key, mode, finalweight, first_view_only):
        """Roll ``n`` actions on this engine and reduce them against ``goal`` -> device rows
        ``[n, score | per view | cost per step]``."""
        ncam, T = self.n_cam, self.sequence_length - self.n_context
        goal_dev = self._goal_on_device(goal, goal_key)

        def reduce(c_s, c_pv, c_cps):
            _lib.check(self._libh.vf_goal_image_scores(
                self._handle, goal_dev.data_ptr(), mode, ctypes.c_float(finalweight), int(bool(first_view_only)),
                c_s.data_ptr(), c_pv.data_ptr(), c_cps.data_ptr(), self._stream()))

        return self._roll_and_reduce(ctx_p, seqs, n, lo, (1, ncam, ncam * T), reduce)

    def split_goal_rows(self, rows_np):
        """Host rows of the goal-image cost -> (scores [M], per view [M, ncam], cost per step [M, ncam, T])."""
        ncam, T = self.n_cam, self.sequence_length - self.n_context
        M = rows_np.shape[0]
        return (np.ascontiguousarray(rows_np[:, 0]), np.ascontiguousarray(rows_np[:, 1:1 + ncam]),
                np.ascontiguousarray(rows_np[:, 1 + ncam:]).reshape(M, ncam, T))

    def score_goal_image_device(self, context, actions_dev, goal_image, steps='last', finalweight=10., first_view_only=False,
                                goal_key=None):
        """``score_goal_image`` without the gather, as ``score_device`` is ``score`` without it: roll ``actions_dev`` - a
        contiguous float32 tensor ``[M, T, adim]`` on this engine's device - and return the device float64 ``scores [M]``.
        Only enqueues (the context and goal uploads aside); the caller checks the downloaded scores with ``_check_scores``.
        Chunked by ``run_batch_size``; the last chunk stays resident for ``render_plans``.  The whole rows
        ``[M, score | per view | cost per step]`` stay in ``last_goal_rows_dev`` (``split_goal_rows`` reads them on the host).
        ValueError: ``frame_score_device_refusal``.  A frames-only engine serves."""
        reason = self.frame_score_device_refusal()
        if reason:
            raise ValueError(reason)
        goal, mode = self._check_goal_cost(goal_image, steps)
        M = self._check_actions_dev(actions_dev)
        with self._torch.cuda.device(self.device):
            ctx_p, seqs = self._prepare_device(self._centre_context(context), actions_dev)
            self._last_prepared = (ctx_p, seqs, M)
            rows = self._goal_rows(ctx_p, seqs, M, 0, goal, goal_key, mode, finalweight, first_view_only)
            self.last_goal_rows_dev = rows
            return rows[:, 0].contiguous()

    # ------------------------------------------------------------------ learned cost (frame scorer)
    def _scorer_here(self, scorer):
        """``scorer`` if it lives on this engine's device, else its cached copy here (one scorer per lane device)."""
        if scorer.device == self.device:
            return scorer
        hit = self._lane_scorers.get(id(scorer))
        if hit is None or hit[0] is not scorer:         # (the entry keeps the scorer alive, so its id stays its own)
            hit = (scorer, scorer.clone_to(self.device))
            self._lane_scorers[id(scorer)] = hit
            while len(self._lane_scorers) > 4:          # a handful of scorers (two heads, a swap); older copies are freed
                self._lane_scorers.pop(next(iter(self._lane_scorers)))
        return hit[1]

    def score_resident_frames(self, scorer, goal_enc=None, finalweight=100.):
        """Score the frames of this engine's LAST rollout chunk again, head outputs included -> (scores [A], cost per
        step [A, T], head outputs [B, T, ncam, D]) on the host; A = B / n_draws.  For tests and measurements."""
        torch = self._torch
        T = self.sequence_length - self.n_context
        A, B = self._last_M, self._last_M * self.n_draws
        scorer = self._scorer_here(scorer)
        with torch.cuda.device(self.device):
            goal_dev = None if goal_enc is None else torch.from_numpy(np.ascontiguousarray(goal_enc, np.float32)).to(self.device)
            s = torch.empty(A, dtype=torch.float64, device=self.device)
            cps = torch.empty((A, T), dtype=torch.float64, device=self.device)
            out = torch.empty((B, T, self.n_cam, scorer.cfg.out_dim), dtype=torch.float32, device=self.device)
            _lib.check(self._libh.vf_scorer_scores(
                scorer._handle, self._handle, None if goal_dev is None else goal_dev.data_ptr(),
                ctypes.c_float(finalweight), s.data_ptr(), cps.data_ptr(), out.data_ptr(), self._stream()))
            return s.cpu().numpy(), cps.cpu().numpy(), out.cpu().numpy()

    @_scoring_entry
    def score_frames(self, context, inputs, scorer, goal_enc=None, finalweight=100.):
        """Fused rollout + learned cost (reference ``policy/cem_controllers/variants/classifier_controller.py:94-105``,
        ``nce_cost_controller.py:90-103``): every predicted frame goes through ``scorer`` (a ``HipFrameScorer``) where
        it lies in the engine, and only score rows leave the GPU.  Returns ``scores[M]`` float64;
        ``last_frame_cost_per_step`` ``[M, T]`` keeps the per-step cost summed over views (averaged over latent draws).

        Classifier head: ``-log(p_success + 1e-5)``; embedding head: ``-<goal_enc, frame embedding>`` with ``goal_enc
        [ncam, D]`` from ``scorer.goal_enc(goal, start)``.  Both are SUMMED over views, then weighted over time by
        ``_weight_scores`` (``finalweight >= 0``: ``w = (1, ..., 1, finalweight)``; ``< 0``: the last step alone).

        Sharding, chunking, lanes and latent draws are those of ``score`` (with ``n_gpus > 1`` the scorer is copied to
        every lane's device once).  As in ``score_goal_image`` the image centre stands in for the goal pixels and
        the distribution context the rollout entry wants."""
        T = self.sequence_length - self.n_context
        goal_enc = self._check_scorer(scorer, goal_enc)
        actions = self._check_actions(inputs['actions'])
        M = actions.shape[0]
        ctx_p, seqs = self._prepare(self._centre_context(context), actions)
        self._last_prepared = (ctx_p, seqs, M)

        def rows_of(lane, share, n, lo):
            return lane._frame_rows(ctx_p, share, n, lo, scorer, goal_enc, finalweight)

        rows_np = score_rows(self, seqs, M, 1 + T, rows_of)
        self.last_frame_cost_per_step = np.ascontiguousarray(rows_np[:, 1:])
        return np.ascontiguousarray(rows_np[:, 0])

    def _check_scorer(self, scorer, goal_enc):
        """The argument checks of the learned-cost entries -> ``goal_enc`` as the kernel takes it (None: classifier head)."""
        c, ncam = self.cfg, self.n_cam
        if (scorer.cfg.height, scorer.cfg.width, scorer.n_cam) != (c.height, c.width, ncam):
            raise ValueError('the scorer is built for %dx%d, %d view(s); the predictor rolls %dx%d, %d view(s)'
                             % (scorer.cfg.height, scorer.cfg.width, scorer.n_cam, c.height, c.width, ncam))
        if scorer.cfg.head != 'embedding':
            return None
        if goal_enc is None:
            raise ValueError('the embedding head needs goal_enc [ncam, D]')
        goal_enc = np.ascontiguousarray(goal_enc, dtype=np.float32)
        if goal_enc.shape != (ncam, scorer.cfg.out_dim):
            raise ValueError('goal_enc must be [%d, %d], got %s' % (ncam, scorer.cfg.out_dim, goal_enc.shape))
        return goal_enc

    def _frame_rows(self, ctx_p, seqs, n, lo, scorer, goal_enc, finalweight):
        """Roll ``n`` actions on this engine and score their frames with ``scorer`` -> device rows
        ``[n, score | cost per step]``."""
        T = self.sequence_length - self.n_context
        here = self._scorer_here(scorer)
        goal_dev = None if goal_enc is None else self._torch.from_numpy(goal_enc).to(self.device)

        def reduce(c_s, c_cps):
            _lib.check(self._libh.vf_scorer_scores(
                here._handle, self._handle, None if goal_dev is None else goal_dev.data_ptr(),
                ctypes.c_float(finalweight), c_s.data_ptr(), c_cps.data_ptr(), None, self._stream()))

        return self._roll_and_reduce(ctx_p, seqs, n, lo, (1, T), reduce)

    def score_frames_device(self, context, actions_dev, scorer, goal_enc=None, finalweight=100.):
        """``score_frames`` without the gather: roll ``actions_dev`` - a contiguous float32 tensor ``[M, T, adim]`` on this
        engine's device - and return the device float64 ``scores [M]``.  Only enqueues (the context and ``goal_enc`` uploads
        aside); the caller checks the downloaded scores with ``_check_scores``.  Chunked by ``run_batch_size``; the last chunk
        stays resident for ``render_plans``.  The whole rows ``[M, score | cost per step]`` stay in ``last_frame_rows_dev``.
        ValueError: ``frame_score_device_refusal``.  A frames-only engine serves."""
        reason = self.frame_score_device_refusal()
        if reason:
            raise ValueError(reason)
        goal_enc = self._check_scorer(scorer, goal_enc)
        M = self._check_actions_dev(actions_dev)
        with self._torch.cuda.device(self.device):
            ctx_p, seqs = self._prepare_device(self._centre_context(context), actions_dev)
            self._last_prepared = (ctx_p, seqs, M)
            rows = self._frame_rows(ctx_p, seqs, M, 0, scorer, goal_enc, finalweight)
            self.last_frame_rows_dev = rows
            return rows[:, 0].contiguous()

    # ------------------------------------------------------------------ in-process multi-GPU (n_gpus > 1)
    def _gather_lane_rows(self, packed, M):
        """The lanes' device rows (lane order, any width) -> all ``M`` rows on the host."""
        rows = None
        if self._use_rccl:
            try:
                rows = self._gather_rccl(packed, M)
            except _lib.VfError as e:
                if self.gather != 'auto':
                    raise
                # 'auto' promises scores, not a transport: say so once and gather through the host from now on
                print('HipVPredEvaluation: grouped RCCL all-gather unavailable (%s); gathering score rows through '
                      'the host' % e)
                self._use_rccl = False
        if rows is None:
            rows = np.concatenate([p.cpu().numpy() for p in packed], axis=0)
        return rows

    def _gather_rccl(self, packed, M):
        """One grouped RCCL all-gather over the lanes' devices (padded to equal rows); lane 0's copy goes to the host."""
        torch, n = self._torch, len(self._lanes)
        P = ctypes.c_void_p
        if self._comms is None:
            devs = (ctypes.c_int32 * n)(*[l.device_index for l in self._lanes])
            comms = (P * n)()
            _lib.check(self._libh.vf_comm_init_all(n, devs, comms))
            self._comms = [P(c) for c in comms]
        sizes = [p.shape[0] for p in packed]
        width, cols = max(sizes), packed[0].shape[1]
        local, full = [], []
        for lane, p in zip(self._lanes, packed):
            with torch.cuda.device(lane.device):
                buf = torch.zeros((width, cols), dtype=torch.float64, device=lane.device)
                buf[:p.shape[0]] = p
                local.append(buf)
                full.append(torch.empty((n * width, cols), dtype=torch.float64, device=lane.device))
        arr = lambda items: (P * n)(*items)
        with torch.cuda.device(self.device):    # (the library also puts the calling thread's device back itself)
            _lib.check(self._libh.vf_allgather_scores_group(
                n, arr([l._handle for l in self._lanes]), arr(self._comms), arr([P(t.data_ptr()) for t in local]),
                width * cols, arr([P(t.data_ptr()) for t in full]), arr([l._stream() for l in self._lanes])))
        with torch.cuda.device(self.device):
            out = full[0].cpu().numpy().reshape(n, width, cols)
        for lane in self._lanes[1:]:        # every lane's collective has completed before its buffers are released
            torch.cuda.synchronize(lane.device)
        return np.concatenate([out[i, :sizes[i]] for i in range(n)], axis=0)

    def set_collective_timing(self, enable):
        """Bracket every score all-gather with HIP events on the stream the collective is ordered on (the current
        stream of this rank's device: c10d makes it wait for the RCCL stream before the call returns) so a bench line
        can show what the one collective of a CEM iteration costs.  ``collective_stats()`` reads them."""
        self._coll_events = [] if enable else None

    def collective_stats(self):
        """-> {'calls', 'mean_ms', 'max_ms', 'bytes_per_rank'} of the all-gathers since ``set_collective_timing(True)``."""
        ev = getattr(self, '_coll_events', None) or []
        if not ev:
            return {'calls': 0, 'mean_ms': None, 'max_ms': None, 'bytes_per_rank': None}
        self._torch.cuda.synchronize(self.device)
        ms = [a.elapsed_time(b) for a, b, _ in ev]
        return {'calls': len(ms), 'mean_ms': float(np.mean(ms)), 'max_ms': float(np.max(ms)),
                'bytes_per_rank': int(ev[-1][2])}

    def fetch_pixel_distributions(self, sample_index):
        """Normalised distributions ``[T, ncam, H, W, ndesig]`` of one action of the last ``score()`` call (its first
        latent draw) - what ``predictor_propagation`` feeds back as the next context (reference
        ``pixel_cost_controller.py:161-165``, where all predicted distributions sit on the host).

        Here only the chunk rolled last stays resident per engine.  The engine that still holds the sample exports
        it (under ``torch.distributed`` a small all-reduce hands it to the other ranks).  A sample nobody holds any
        more - ``num_samples > vpred_batch_size``, e.g. the reference's 600-sample RoboNet configs - is simply rolled
        again, alone: a sample's arithmetic does not depend on the batch it is rolled in, so the result is
        bit-identical to the first pass, and every rank can do it locally without a collective."""
        self._refuse_frames_only('fetch_pixel_distributions')
        torch, c = self._torch, self.cfg
        T = self.sequence_length - self.n_context
        rank, world = _dist_info()
        prepared = getattr(self, '_last_prepared', None)
        if prepared is not None and not 0 <= sample_index < prepared[2]:
            raise IndexError('sample %d outside the last scoring call (%d actions)' % (sample_index, prepared[2]))
        for lane in (self._lanes or [])[1:]:        # in-process multi-GPU: the lane that rolled it exports it
            if 0 <= sample_index - lane._last_lo < lane._last_M:
                return lane.fetch_pixel_distributions(sample_index)
        local = sample_index - self._last_lo
        have = 0 <= local < self._last_M
        out = torch.zeros((T, self.n_cam, c.height, c.width, c.ndesig), dtype=torch.float32, device=self.device)
        if have:
            with torch.cuda.device(self.device):
                _lib.check(self._libh.vf_export(self._handle, int(local) * self.n_draws, 1, None, out.data_ptr(),
                                                None, self._stream()))
        if world > 1:
            import torch.distributed as dist
            # the "somebody holds it" flag travels with the data (one extra element)
            flat = torch.cat([out.reshape(-1), torch.tensor([1.0 if have else 0.0], device=self.device)])
            if dist.get_backend() == 'gloo':
                host = flat.cpu()
                dist.all_reduce(host)
                flat = host.to(self.device)
            else:
                dist.all_reduce(flat)   # exactly one rank holds the sample, the others add zeros
            if float(flat[-1].item()) >= 0.5:
                return flat[:-1].reshape(out.shape).cpu().numpy()
            have = False                # nobody holds it: every rank rolls it again below (identical results)
        if have:
            return out.cpu().numpy()
        if prepared is None:
            raise IndexError('sample %d is not resident (last chunk holds [%d, %d))'
                             % (sample_index, self._last_lo, self._last_lo + self._last_M))
        return self._reroll_one(sample_index, out)

    def _reroll(self, indices):
        """Roll the actions ``indices`` of the last scoring call again as ONE batch (``len(indices) * n_draws`` sequences of
        ``_last_prepared``, at most ``run_batch_size``) -> their device scores.  Row ``i * n_draws`` of the resident batch is
        then the first draw of ``indices[i]``.  Call under this engine's device."""
        torch, nd = self._torch, self.n_draws
        ctx_p, seqs, _ = self._last_prepared
        ntask = self.n_cam * self.cfg.ndesig
        n = len(indices)
        rows = (np.asarray(indices, dtype=np.int64)[:, None] * nd + np.arange(nd)[None]).reshape(-1)
        self._set_context(ctx_p)
        if torch.is_tensor(seqs):       # the last call was score_device: its sequences never left the device
            seq = seqs[torch.from_numpy(rows).to(self.device)].contiguous()
        else:
            seq = torch.from_numpy(np.ascontiguousarray(np.asarray(seqs)[rows], dtype=np.float32)).to(self.device)
        # (a frames-only rollout writes no pixel scores: zeros stand in, the failure word is read instead)
        scores = (torch.zeros if self.frames_only else torch.empty)(n, dtype=torch.float64, device=self.device)
        per_task = torch.empty((n, ntask), dtype=torch.float64, device=self.device)
        self._rollout_chunk(seq, np.zeros((self.n_cam, self.cfg.ndesig, 2), np.int32), 1.0, scores, per_task)
        # what is resident now is not a range of the scoring call, unless it is one action.  Under torch.distributed
        # EVERY rank may have just rolled it: nobody may claim to be "the" holder afterwards (the fetch's all-reduce
        # adds the holders' copies), so the ranks keep nothing resident
        alone = n == 1 and _dist_info()[1] == 1
        self._last_lo, self._last_M = int(indices[0]), (1 if alone else 0)
        return scores

    def _reroll_one(self, sample_index, out):
        """Roll action ``sample_index`` of the last scoring call again (its ``n_draws`` sequences, alone) and export
        the first draw's distributions into ``out``."""
        with self._torch.cuda.device(self.device):
            scores = self._reroll([sample_index])
            _lib.check(self._libh.vf_export(self._handle, 0, 1, None, out.data_ptr(), None, self._stream()))
            self._check_scores(scores.cpu().numpy())
            return out.cpu().numpy()

    # ------------------------------------------------------------------ plan visualisation
    def _render_resident(self, rows, lut_dev, frames, distributions):
        """``vf_render_plans`` on the rolled sequences ``rows`` of this engine's resident batch -> device uint8 tensors
        (frames ``[K, ncam, T, H, W, 3]`` or None, distributions ``[K, ncam, ndesig, T, H, W, 3]`` or None)."""
        torch, c = self._torch, self.cfg
        T, K = self.sequence_length - self.n_context, len(rows)
        seq = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
        f = torch.empty((K, self.n_cam, T, c.height, c.width, 3), dtype=torch.uint8, device=self.device) if frames else None
        d = torch.empty((K, self.n_cam, c.ndesig, T, c.height, c.width, 3), dtype=torch.uint8,
                        device=self.device) if distributions else None
        _lib.check(self._libh.vf_render_plans(self._handle, seq.data_ptr(), K, lut_dev.data_ptr(),
                                              f.data_ptr() if frames else None, d.data_ptr() if distributions else None,
                                              self._stream()))
        return f, d

    def render_plans(self, indices, lut=None, frames=True, distributions=True):
        """The plan page's pictures (reference ``pixel_cost_controller.py:107-126``) of K actions of the last ``score()``
        / ``score_goal_image()`` call (with latent draws: their first draw), rendered on the GPU: ``{'frames': uint8
        [K, ncam, T, H, W, 3], 'distributions': uint8 [K, ncam, ndesig, T, H, W, 3]}`` (the keys asked for).  Frames are
        ``trunc(frame * 255)``, every distribution plane is coloured against its own maximum through ``lut`` (uint8
        ``[256, 3]``, default viridis) - the arithmetic of ``visualizer/colormap.py``, bit for bit.

        When this engine still holds all K (one engine and ``M <= run_batch_size``: the reference default) nothing is
        rolled.  Otherwise - chunked calls, lanes, ``torch.distributed`` ranks - the K actions are rolled again as one
        batch: a sample's arithmetic does not depend on its batch, so the bytes are the same, and every rank does it
        locally without a collective."""
        from visual_foresight_amd.policy.cem_controllers.visualizer.colormap import check_lut
        torch, nd = self._torch, self.n_draws
        prepared = self._last_prepared
        if prepared is None:
            raise IndexError('render_plans follows a score() / score_goal_image() call')
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.size == 0 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError('indices must be a non-empty 1-d integer sequence, got %r' % (indices,))
        if not (frames or distributions):
            raise ValueError('nothing to render: frames and distributions are both off')
        if distributions:
            self._refuse_frames_only('render_plans(distributions=True)')
        if idx.min() < 0 or idx.max() >= prepared[2]:
            raise IndexError('indices %s outside the last scoring call (%d actions)' % (idx.tolist(), prepared[2]))
        if len(np.unique(idx)) != idx.size:
            raise ValueError('indices repeat: %s' % (idx.tolist(),))
        parts = []
        with torch.cuda.device(self.device):
            lut_dev = torch.from_numpy(np.array(check_lut(lut))).to(self.device)
            local = idx - self._last_lo
            if local.min() >= 0 and local.max() < self._last_M:
                parts.append(self._render_resident(local * nd, lut_dev, frames, distributions))
            else:
                bs = self.run_batch_size // nd
                rolled = []
                for g0 in range(0, idx.size, bs):
                    group = idx[g0:g0 + bs]
                    rolled.append(self._reroll(group))
                    parts.append(self._render_resident(np.arange(group.size) * nd, lut_dev, frames, distributions))
                self._check_scores(torch.cat(rolled).cpu().numpy())
                if self.frames_only:
                    self._check_status()
            out = {}
            if frames:
                out['frames'] = torch.cat([p[0] for p in parts]).cpu().numpy()
            if distributions:
                out['distributions'] = torch.cat([p[1] for p in parts]).cpu().numpy()
        return out

    # ------------------------------------------------------------------ registration
    def register(self, current, reference, flow, pix, region=0, clip_sub=1, want_warped=False):
        """Device side of ``get_warp_err`` (reference ``register_gtruth_controller.py:113-173``).

        current, reference ``[ncam, H, W, 3]`` float images, flow ``[ncam, H, W, 2]`` (dx, dy) of the
        registration network - each a NumPy array or a float tensor on this predictor's device, which is used
        without a host round trip (``HipRegistrationNet.flow_device``) - pix ``[ncam, ntask, 2]`` (row, col) in the reference image.  Returns
        ``desig [ncam, ntask, 2]`` (row, col in the current frame), ``err [ncam, ntask]`` and, on request,
        the warped frame ``[ncam, H, W, 3]`` and the warp points ``[ncam, H, W, 2]`` (x, y).
        """
        torch, c = self._torch, self.cfg

        def as_input(a):        # device tensors (a registration net's flow) are used where they lie, the rest becomes NumPy
            if torch.is_tensor(a) and a.is_cuda:
                if a.device != self.device:
                    raise ValueError('register: a tensor on %s was given, the predictor registers on %s' % (a.device, self.device))
                return a.to(torch.float32).contiguous()
            return np.ascontiguousarray(a, dtype=np.float32)

        cur, ref, fl = as_input(current), as_input(reference), as_input(flow)
        px = np.ascontiguousarray(pix, dtype=np.int32).reshape(self.n_cam, -1, 2)
        # at the model's size vf_register; at the camera's (camera_height / camera_width) vf_register_hw, whose pixels and
        # results are in camera coordinates (the reference registers at the agent's resolution, :121-128,144-155)
        size = (c.height, c.width)
        if self.camera_size is not None and tuple(cur.shape[1:3]) == self.camera_size:
            size = self.camera_size
        if tuple(cur.shape) != (self.n_cam,) + size + (3,) or tuple(ref.shape) != tuple(cur.shape) or \
                tuple(fl.shape) != (self.n_cam,) + size + (2,):
            raise ValueError('register: need [ncam, H, W, 3] images and a [ncam, H, W, 2] flow field%s'
                             % (' at the model size %d x %d or the camera size %d x %d' % ((c.height, c.width) + self.camera_size)
                                if self.camera_size is not None else ''))
        entry = (self._libh.vf_register, (self._handle,)) if size == (c.height, c.width) else \
            (self._libh.vf_register_hw, (self._handle,) + size)
        ntask = px.shape[1]
        with torch.cuda.device(self.device):
            d_cur, d_ref, d_fl, d_px = (a if torch.is_tensor(a) else torch.from_numpy(a).to(self.device)
                                        for a in (cur, ref, fl, px))
            desig = torch.empty((self.n_cam, ntask, 2), dtype=torch.float32, device=self.device)
            err = torch.empty((self.n_cam, ntask), dtype=torch.float32, device=self.device)
            warped = torch.empty_like(d_cur) if want_warped else None
            pts = torch.empty_like(d_fl) if want_warped else None
            _lib.check(entry[0](
                *entry[1], d_cur.data_ptr(), d_ref.data_ptr(), d_fl.data_ptr(), d_px.data_ptr(), ntask,
                int(region), int(clip_sub), warped.data_ptr() if want_warped else None,
                pts.data_ptr() if want_warped else None, desig.data_ptr(), err.data_ptr(), self._stream()))
            out = desig.cpu().numpy().astype(np.float64), err.cpu().numpy().astype(np.float64)
            if want_warped:
                out = out + (warped.cpu().numpy(), pts.cpu().numpy())
        return out

    def predictor_func(self):
        """The legacy boundary (reference ``video_prediction/setup_predictor.py:164-200``): a callable

            ``f(input_images=, input_one_hot_images=, input_state=, input_actions=) -> (gen_images, gen_distrib, gen_states)``

        as ``rollout_predictions`` (``pred_util.py:21-48``) drives it.  ``input_images`` is the batch-1
        float context ``[1, n_context, 1, H, W, 3]`` in [0, 1] (``get_context``), ``input_state``
        ``[1, n_context, sdim]``, ``input_one_hot_images`` ``[1, n_context, 1, H, W, ndesig]`` or None and
        ``input_actions`` ``[B, sequence_length (or sequence_length - 1), adim]`` whose first
        ``n_context - 1`` steps are the executed actions (identical for every row, as the reference
        tiles them).  Returns the ``sequence_length - n_context`` future frames
        ``[B, T, 1, H, W, 3]``, distributions ``[B, T, 1, H, W, ndesig]`` (None without input
        distributions) and states ``[B, T, sdim]``.
        """
        nc, c = self.n_context, self.cfg
        T = self.sequence_length - nc
        if self.n_cam != 1 or self.n_draws != 1:
            raise NotImplementedError('the legacy predictor_func boundary is single-view, deterministic')

        def predictor_func(input_images=None, input_one_hot_images=None, input_state=None, input_actions=None):
            acts = np.asarray(input_actions, dtype=np.float64)
            if acts.ndim != 3 or acts.shape[1] not in (self.sequence_length, self.sequence_length - 1):
                raise ValueError('input_actions must be [B, %d, %d], got %s'
                                 % (self.sequence_length, c.adim, acts.shape))
            ctx_actions, future = acts[:, :nc - 1], acts[:, nc - 1:nc - 1 + T]
            padding = ~acts.reshape(acts.shape[0], -1).any(axis=1)      # zero rows of a padded last chunk
            if nc > 1 and not np.all((ctx_actions == ctx_actions[:1]).all(axis=(1, 2)) | padding):
                raise ValueError('the first n_context-1 actions are context and must be the same for every row')
            frames = np.asarray(input_images)[0]
            if frames.dtype != np.uint8:        # get_context hands over float frames in [0, 1]
                frames = np.rint(frames * 255.).astype(np.uint8)
            if self.frames_only:
                if input_one_hot_images is not None:
                    raise ValueError('this predictor is frames-only (designated_pixel_count 0 / no_pix_distrib): '
                                     'input_one_hot_images must be None')
                distrib = None
            elif input_one_hot_images is None:
                distrib = np.zeros((nc, 1, c.height, c.width, c.ndesig), np.float32)
                distrib[:, :, 0, 0, :] = 1.0
            else:
                distrib = np.asarray(input_one_hot_images, dtype=np.float32)[0]
            context = {'context_frames': frames, 'context_states': np.asarray(input_state)[0],
                       'context_actions': ctx_actions[0] if nc > 1 else np.zeros((1, c.adim)),
                       'context_pixel_distributions': distrib}
            if distrib is None:
                del context['context_pixel_distributions']
            out = self(context, {'actions': future})
            return (out['predicted_frames'],
                    None if input_one_hot_images is None else out['predicted_pixel_distributions'],
                    out['predicted_states'])

        return predictor_func

    def __call__(self, context, inputs):
        """Reference-compatible path: materialise all predicted frames and distributions on the host
        (``[M, T, ncam, H, W, C]``; with latent draws, the first draw of every action)."""
        actions = self._check_actions(inputs['actions'])
        context, seqs = self._prepare(context, actions)
        self._last_prepared = (context, seqs, actions.shape[0])
        if self._lanes:     # lane i materialises its contiguous shard (one lane after the other: the D2H dominates)
            nd = self.n_draws
            parts = [lane._materialise(context, seqs[lo * nd:hi * nd], hi - lo, lo)
                     for lane, lo, hi in self._lane_shares(actions.shape[0]) if hi > lo]
            if not parts:       # M == 0: empty arrays of the right shapes
                return self._materialise(context, seqs, 0, 0)
            return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}
        return self._materialise(context, seqs, actions.shape[0], 0)

    def _materialise(self, context, seqs, M, index_base):
        torch, c = self._torch, self.cfg
        T = self.sequence_length - self.n_context
        ncam, nd = self.n_cam, self.n_draws
        frames = np.empty((M, T, ncam, c.height, c.width, 3), np.float32)
        # (frames-only: 'predicted_pixel_distributions' is None - what the reference's predictor_func returns for gen_distrib
        # under no_pix_distrib)
        distrib = None if self.frames_only else np.empty((M, T, ncam, c.height, c.width, c.ndesig), np.float32)
        states = np.empty((M, T, c.sdim), np.float32)
        zero_goal = np.zeros((ncam, c.ndesig, 2), np.int32)
        bs = self.run_batch_size // nd
        with torch.cuda.device(self.device):
            self._set_context(context)
            acts = torch.from_numpy(np.ascontiguousarray(seqs, dtype=np.float32)).to(self.device)
            scores = torch.empty(bs, dtype=torch.float64, device=self.device)
            per_task = torch.empty((bs, ncam * c.ndesig), dtype=torch.float64, device=self.device)
            for c0 in range(0, M, bs):
                c1 = min(c0 + bs, M)
                n = c1 - c0
                self._rollout_chunk(acts[c0 * nd:c1 * nd], zero_goal, 1.0, scores[:n], per_task[:n])
                self._last_lo, self._last_M = index_base + c0, n
                f = torch.empty((n * nd, T, ncam, c.height, c.width, 3), dtype=torch.float32, device=self.device)
                d = None if self.frames_only else torch.empty((n * nd, T, ncam, c.height, c.width, c.ndesig),
                                                              dtype=torch.float32, device=self.device)
                s = torch.empty((n * nd, T, c.sdim), dtype=torch.float32, device=self.device)
                _lib.check(self._libh.vf_export(self._handle, 0, n * nd, f.data_ptr(), None if d is None else d.data_ptr(),
                                                s.data_ptr(), self._stream()))
                frames[c0:c1] = f[::nd].cpu().numpy()
                if d is not None:
                    distrib[c0:c1] = d[::nd].cpu().numpy()
                states[c0:c1] = s[::nd].cpu().numpy()
            if M > 0 and not self.frames_only:
                self._check_scores(scores[:n].cpu().numpy())
            elif M > 0:
                self._check_status()
            else:
                self._last_lo, self._last_M = index_base, 0
        return {'predicted_frames': frames, 'predicted_pixel_distributions': distrib,
                'predicted_states': states}


class FramesOnlyHipVPredEvaluation(HipVPredEvaluation):
    """``HipVPredEvaluation`` with zero designated pixels whatever ``designated_pixel_count`` its hyper-parameters carry:
    the controllers that score predicted FRAMES (``ClassifierController``, ``NCECostController``, ``GoalImController``) pass
    1, because the network used to need a distribution channel.  ``policy['predictor_class'] =
    FramesOnlyHipVPredEvaluation`` selects the frames-only engine without a new policy hyper-parameter - the reference's
    ``no_pix_distrib`` predictor conf."""
    force_frames_only = True


class MultiViewHipPredictor(HipVPredEvaluation):
    """``ncam`` independent single-view networks behind the ``VPredEvaluation`` duck-type (the reference's
    ``IndepMultiSAVPVideoPredictionModel``: one network per view sharing actions and states, outputs stacked on a camera
    axis, ``visual_mpc/video_prediction/vpred_model_interface.py:60-88``).  The engine is the base class's - every view
    of every sample rolls in the SAME persistent launch, per-task scores come back camera-major - this class only fixes
    the construction conventions: ``ncam`` defaults to 2, ``model_path`` is a list of per-view directories or a directory
    with ``view0/``, ``view1/`` ... inside, random-init seeds are ``seed + view``."""

    def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
        hp = dict(hparams)
        hp.setdefault('ncam', 2)
        super(MultiViewHipPredictor, self).__init__(model_path, hp, n_gpus=n_gpus, first_gpu=first_gpu)

    @staticmethod
    def view_context(context, c):
        """The single-view slice of a multi-view context (what one view's network sees)."""
        return {'context_frames': np.asarray(context['context_frames'])[:, c:c + 1],
                'context_pixel_distributions': np.asarray(context['context_pixel_distributions'])[:, c:c + 1],
                'context_actions': context['context_actions'], 'context_states': context['context_states']}
