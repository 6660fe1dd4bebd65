"""ctypes binding of libvf_hip.so (the C ABI declared in include/vf_hip.h).

The library is built in-tree by ``build_library()`` (``hipcc --offload-arch=gfx950``; it
cross-compiles without a GPU).  There is no CPU fallback: ``load_library()`` raises if the
shared object is missing, and every wrapper raises ``VfError`` with ``vf_last_error()`` when
a call fails.
"""
import ctypes
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
LIB_PATH = os.environ.get('VF_LIBRARY') or os.path.join(_HERE, 'libvf_hip.so')     # override: experiments only
SOURCES = [os.path.join(_HERE, 'csrc', f) for f in
           ('vf_engine.hip', 'vf_conv_mfma.h', 'vf_conv_gsplit.h', 'vf_small_kernels.h', 'vf_goal_image.h', 'vf_plan_render.h', 'vf_resize.h', 'vf_cem.h', 'vf_net_conv.h',
            'vf_frame_scorer.h', 'vf_engine_sidenet.inc', 'vf_engine_scorer.inc', 'vf_registration_net.h', 'vf_engine_regnet.inc', 'vf_inverse_model.h', 'vf_engine_invmodel.inc', 'vf_engine_cem.inc', 'vf_persistent.h',
            'vf_conv_bf16x6.h', 'vf_conv_bf16.h', 'vf_fused_top.h', 'vf_fc_tile.h', 'vf_conv_first.h', 'vf_savp3.h', 'vf_engine_savp3.inc')] + \
          [os.path.join(REPO, 'include', 'vf_hip.h')]

# every symbol include/vf_hip.h declares
EXPORTS = ('vf_abi_version', 'vf_last_error', 'vf_weight_count', 'vf_create', 'vf_destroy',
           'vf_load_weights', 'vf_set_context', 'vf_rollout', 'vf_export', 'vf_register',
           'vf_allgather_scores', 'vf_comm_init_all', 'vf_comm_destroy', 'vf_allgather_scores_group',
           'vf_macs_per_sample_step', 'vf_set_profiling', 'vf_get_profile',
           'vf_set_dedup', 'vf_set_persistent', 'vf_set_xcd_queues', 'vf_set_fuse_top', 'vf_device_status',
           'vf_set_phase_stats', 'vf_debug_phase_stats', 'vf_debug_poison_status', 'vf_set_sched_option',
           'vf_ensemble_scores', 'vf_goal_image_scores', 'vf_render_plans',
           'vf_scorer_weight_count', 'vf_scorer_create', 'vf_scorer_destroy', 'vf_scorer_load_weights', 'vf_scorer_embed',
           'vf_scorer_scores',
           'vf_regnet_weight_count', 'vf_regnet_create', 'vf_regnet_destroy', 'vf_regnet_load_weights', 'vf_regnet_flow',
           'vf_invmodel_weight_count', 'vf_invmodel_create', 'vf_invmodel_destroy', 'vf_invmodel_load_weights',
           'vf_invmodel_infer', 'vf_debug_lstm_layer', 'vf_register_hw', 'vf_resize_area',
           'vf_cem_workspace_bytes', 'vf_cem_refit', 'vf_cem_sample',
           'vf_cem_corr_workspace_bytes', 'vf_cem_soft_refit', 'vf_cem_sample_corr', 'vf_cem_sample_fold',
           'vf_cem_sample_autograsp', 'vf_cem_latents', 'vf_cem_fold_latents',
           'vf_set_contexts', 'vf_group_pixel_scores')
ABI_VERSION = 7


class VfError(RuntimeError):
    pass


class VfConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ('height', 'width', 'adim', 'sdim', 'ndesig', 'n_context', 'sequence_length',
                 'num_masks', 'max_batch', 'device', 'precision', 'ncam', 'n_draws', 'arch', 'zdim', 'layer_spec')]


class VfScorerConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('height', 'width', 'ncam', 'head', 'embed_dim', 'max_frames', 'device')] + \
               [('input_scale', ctypes.c_float)]


class VfRegnetConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('height', 'width', 'ncam', 'ch_mult', 'max_pairs', 'device')]


class VfCemConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('nactions', 'repeat', 'adim', 'tail', 'n_elites', 'max_trials', 'rejection',
                                              'zero_first', 'discrete_mask')] + \
               [('seed_lo', ctypes.c_uint32), ('seed_hi', ctypes.c_uint32), ('reserved', ctypes.c_int32)] + \
               [(n, ctypes.c_double * 8) for n in ('rej_lim', 'trunc_lim', 'tail_value')]


class VfCemCorrConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('nactions', 'adim', 'tail', 'n_elites', 'refit_cov', 'has_first_prev')] + \
               [('seed_lo', ctypes.c_uint32), ('seed_hi', ctypes.c_uint32)] + \
               [(n, ctypes.c_double) for n in ('kappa', 'beta_0', 'beta_1')] + \
               [(n, ctypes.c_double * 8) for n in ('std', 'bias', 'first_prev', 'tail_value')]


class VfCemFoldConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('nactions', 'repeat', 'tail', 'n_elites', 'n_scripted', 'reserved')] + \
               [('seed_lo', ctypes.c_uint32), ('seed_hi', ctypes.c_uint32)] + \
               [('start_xy', ctypes.c_double * 2), ('max_shift', ctypes.c_double * 3), ('tail_value', ctypes.c_double * 8)]


class VfCemGripConfig(ctypes.Structure):
    _fields_ = [('mode', ctypes.c_int32), ('reopen', ctypes.c_int32)] + \
               [(n, ctypes.c_double) for n in ('state_z', 'action_norm_factor', 'z_thresh', 'deviation_prob', 'close_cmd',
                                               'open_cmd')]


class VfInvModelConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('height', 'width', 'adim', 'n_context', 'n_actions', 'max_batch', 'device')] + \
               [('input_scale', ctypes.c_float)]


def _hipcc():
    for cand in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise VfError('hipcc not found; cannot build libvf_hip.so')


def library_is_stale():
    if os.environ.get('VF_LIBRARY'):
        return False
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > built for s in SOURCES)


def build_library(force=False, verbose=False):
    """Compile the HIP engine for gfx950 into visual_foresight_amd/libvf_hip.so."""
    if not force and not library_is_stale():
        return LIB_PATH
    cmd = [_hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
           '-o', LIB_PATH + '.tmp', SOURCES[0]]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or proc.returncode:
        print(' '.join(cmd))
        print(proc.stdout)
    if proc.returncode:
        raise VfError('hipcc failed building libvf_hip.so')
    os.replace(LIB_PATH + '.tmp', LIB_PATH)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen libvf_hip.so and declare the prototypes.  Raises VfError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VfError('%s is missing - run `python -c "import __graft_entry__ as g; g.build()"` '
                      '(there is no CPU fallback for the predictor)' % LIB_PATH)
    # PyTorch (the buffer carrier) ships its own copy of the HIP runtime.  It must be the FIRST one this process loads:
    # when libvf_hip.so pulls in /opt/rocm's libamdhip64 before torch has loaded its bundled one, the process ends up
    # with two runtimes and the second reports "no ROCm-capable device" (seen with build() followed by smoke() in one
    # process).  Importing torch here makes the order independent of what the caller did first.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    lib.vf_abi_version.restype = ctypes.c_int
    lib.vf_last_error.restype = ctypes.c_char_p
    lib.vf_weight_count.restype = ctypes.c_size_t
    lib.vf_weight_count.argtypes = [ctypes.POINTER(VfConfig)]
    lib.vf_macs_per_sample_step.restype = ctypes.c_double
    lib.vf_macs_per_sample_step.argtypes = [ctypes.POINTER(VfConfig)]
    lib.vf_create.argtypes = [ctypes.POINTER(VfConfig), ctypes.POINTER(P)]
    lib.vf_destroy.argtypes = [P]
    lib.vf_load_weights.argtypes = [P, P, ctypes.c_size_t]
    lib.vf_set_context.argtypes = [P, P, P, P, P, P]
    lib.vf_set_contexts.argtypes = [P, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P]
    lib.vf_group_pixel_scores.argtypes = [P, P, ctypes.c_float, ctypes.POINTER(ctypes.c_float), P, P, P]
    lib.vf_set_contexts.restype = lib.vf_group_pixel_scores.restype = ctypes.c_int
    lib.vf_rollout.argtypes = [P, P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_float,
                               ctypes.POINTER(ctypes.c_float), P, P, P]
    lib.vf_ensemble_scores.argtypes = [ctypes.POINTER(P), ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                       ctypes.POINTER(ctypes.c_float), P, P, P, P]
    lib.vf_goal_image_scores.argtypes = [P, P, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, P, P, P, P]
    lib.vf_render_plans.argtypes = [P, P, ctypes.c_int32, P, P, P, P]
    lib.vf_scorer_weight_count.restype = ctypes.c_size_t
    lib.vf_scorer_weight_count.argtypes = [ctypes.POINTER(VfScorerConfig), ctypes.c_int32]
    lib.vf_scorer_create.argtypes = [ctypes.POINTER(VfScorerConfig), ctypes.POINTER(P)]
    lib.vf_scorer_destroy.argtypes = [P]
    lib.vf_scorer_load_weights.argtypes = [P, ctypes.c_int32, P, ctypes.c_size_t]
    lib.vf_scorer_embed.argtypes = [P, ctypes.c_int32, P, ctypes.c_int32, P, P]
    lib.vf_scorer_scores.argtypes = [P, P, P, ctypes.c_float, P, P, P, P]
    lib.vf_regnet_weight_count.restype = ctypes.c_size_t
    lib.vf_regnet_weight_count.argtypes = [ctypes.POINTER(VfRegnetConfig)]
    lib.vf_regnet_create.argtypes = [ctypes.POINTER(VfRegnetConfig), ctypes.POINTER(P)]
    lib.vf_regnet_destroy.argtypes = [P]
    lib.vf_regnet_load_weights.argtypes = [P, P, ctypes.c_size_t]
    lib.vf_regnet_flow.argtypes = [P, P, P, ctypes.c_int32, P, P]
    lib.vf_invmodel_weight_count.restype = ctypes.c_size_t
    lib.vf_invmodel_weight_count.argtypes = [ctypes.POINTER(VfInvModelConfig)]
    lib.vf_invmodel_create.argtypes = [ctypes.POINTER(VfInvModelConfig), ctypes.POINTER(P)]
    lib.vf_invmodel_destroy.argtypes = [P]
    lib.vf_invmodel_load_weights.argtypes = [P, P, ctypes.c_size_t]
    lib.vf_invmodel_infer.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, P]
    lib.vf_register.argtypes = [P, P, P, P, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P]
    lib.vf_register_hw.argtypes = [P, ctypes.c_int32, ctypes.c_int32] + lib.vf_register.argtypes[1:]
    lib.vf_resize_area.argtypes = [ctypes.c_int32, P, P] + [ctypes.c_int32] * 7 + [P]
    lib.vf_cem_workspace_bytes.restype = ctypes.c_size_t
    lib.vf_cem_workspace_bytes.argtypes = [ctypes.POINTER(VfCemConfig)]
    lib.vf_cem_refit.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemConfig), P, P, ctypes.c_int32, P, P, P, P, P]
    lib.vf_cem_sample.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemConfig), P, ctypes.c_uint32, ctypes.c_int32, P, P, P, P]
    lib.vf_cem_refit.restype = lib.vf_cem_sample.restype = ctypes.c_int
    lib.vf_cem_corr_workspace_bytes.restype = ctypes.c_size_t
    lib.vf_cem_corr_workspace_bytes.argtypes = [ctypes.POINTER(VfCemCorrConfig)]
    lib.vf_cem_soft_refit.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemCorrConfig), P, P, ctypes.c_int32, P, P, P, P, P]
    lib.vf_cem_sample_corr.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemCorrConfig), P, ctypes.c_uint32, ctypes.c_int32, P, P]
    lib.vf_cem_soft_refit.restype = lib.vf_cem_sample_corr.restype = ctypes.c_int
    lib.vf_cem_sample_fold.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemFoldConfig), P, ctypes.c_uint32, ctypes.c_int32, P, P]
    lib.vf_cem_sample_fold.restype = ctypes.c_int
    lib.vf_cem_sample_autograsp.argtypes = [ctypes.c_int32, ctypes.POINTER(VfCemConfig), ctypes.POINTER(VfCemGripConfig), P,
                                            ctypes.c_uint32, ctypes.c_int32, P, P, P, P, P, P]
    lib.vf_cem_sample_autograsp.restype = ctypes.c_int
    lib.vf_cem_latents.argtypes = [ctypes.c_int32] + [ctypes.c_uint32] * 3 + [ctypes.c_int32] * 3 + [P, P]
    lib.vf_cem_fold_latents.argtypes = [ctypes.c_int32, P, P] + [ctypes.c_int32] * 5 + [P, P]
    lib.vf_cem_latents.restype = lib.vf_cem_fold_latents.restype = ctypes.c_int
    lib.vf_allgather_scores.argtypes = [P, P, P, ctypes.c_int32, P, P]
    lib.vf_comm_init_all.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(P)]
    lib.vf_comm_destroy.argtypes = [P]
    lib.vf_allgather_scores_group.argtypes = [ctypes.c_int32, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P),
                                              ctypes.c_int32, ctypes.POINTER(P), ctypes.POINTER(P)]
    lib.vf_set_phase_stats.argtypes = [P, ctypes.c_int32]
    lib.vf_debug_phase_stats.argtypes = [P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    lib.vf_debug_poison_status.argtypes = [P]
    lib.vf_debug_lstm_layer.argtypes = [P, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P]
    lib.vf_export.argtypes = [P, ctypes.c_int32, ctypes.c_int32, P, P, P, P]
    lib.vf_set_profiling.argtypes = [P, ctypes.c_int32]
    lib.vf_get_profile.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.vf_set_dedup.argtypes = [P, ctypes.c_int32]
    lib.vf_set_dedup.restype = ctypes.c_int
    lib.vf_set_persistent.argtypes = [P, ctypes.c_int32]
    lib.vf_set_xcd_queues.argtypes = [P, ctypes.c_int32]
    lib.vf_set_fuse_top.argtypes = [P, ctypes.c_int32]
    lib.vf_set_sched_option.argtypes = [P, ctypes.c_int32, ctypes.c_int32]
    lib.vf_set_sched_option.restype = ctypes.c_int
    lib.vf_set_fuse_top.restype = ctypes.c_int
    lib.vf_set_xcd_queues.restype = ctypes.c_int
    lib.vf_device_status.argtypes = [P, ctypes.POINTER(ctypes.c_int32)]
    lib.vf_set_persistent.restype = lib.vf_device_status.restype = ctypes.c_int
    lib.vf_set_profiling.restype = lib.vf_get_profile.restype = ctypes.c_int
    for name in ('vf_create', 'vf_destroy', 'vf_load_weights', 'vf_set_context', 'vf_rollout', 'vf_ensemble_scores',
                 'vf_goal_image_scores', 'vf_render_plans', 'vf_scorer_create', 'vf_scorer_destroy',
                 'vf_scorer_load_weights', 'vf_scorer_embed', 'vf_scorer_scores',
                 'vf_regnet_create', 'vf_regnet_destroy', 'vf_regnet_load_weights', 'vf_regnet_flow',
                 'vf_invmodel_create', 'vf_invmodel_destroy', 'vf_invmodel_load_weights', 'vf_invmodel_infer',
                 'vf_export', 'vf_register', 'vf_register_hw', 'vf_resize_area', 'vf_allgather_scores', 'vf_comm_init_all', 'vf_comm_destroy',
                 'vf_allgather_scores_group', 'vf_set_phase_stats',
                 'vf_debug_phase_stats', 'vf_debug_poison_status', 'vf_debug_lstm_layer'):
        getattr(lib, name).restype = ctypes.c_int
    if lib.vf_abi_version() != ABI_VERSION:
        raise VfError('libvf_hip.so ABI version %d, expected %d (stale build? run __graft_entry__.build())'
                      % (lib.vf_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VfError('libvf_hip error %d: %s' % (rc, load_library().vf_last_error().decode()))
