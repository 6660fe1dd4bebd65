// vf_engine_cem.inc - host side of the device CEM (vf_cem.h; include/vf_hip.h "Device-resident CEM iteration"): the config
// checks, the kernel parameter builders, the argument checks and the ten handle-free vf_cem_* entries.  Included at the end
// of vf_engine.hip, ahead of the side networks' files: cem_fold_latents_kernel<> is instantiated here, and the device
// functions of the code object follow the order of instantiation.  Every entry is defined once: its refusals are host
// work only (nothing of the device is touched before they are through), and behind them the -DVF_HOST_SELFTEST build
// launches nothing.

namespace vf {

static int cem_config_check(const vf_cem_config *c, const char *who) {
    const std::string w(who);
    if (!c) return fail(VF_ERR_INVALID, w + ": null cfg");
    if (c->nactions < 1 || c->repeat < 1 || c->adim < 1 || c->tail < 0 || c->adim + c->tail > kCemMaxWidth)
        return fail(VF_ERR_INVALID, w + ": need nactions >= 1, repeat >= 1, adim >= 1, tail >= 0 and adim + tail <= 8");
    if ((long long)c->nactions * c->adim > kCemMaxD)
        return fail(VF_ERR_INVALID, w + ": D = nactions * adim = " + std::to_string((long long)c->nactions * c->adim) + " exceeds 128");
    if ((long long)c->nactions * c->repeat > (1 << 16))
        return fail(VF_ERR_INVALID, w + ": T = nactions * repeat exceeds 2^16");
    if (c->n_elites < 2 || c->n_elites > kCemMaxK)
        return fail(VF_ERR_INVALID, w + ": n_elites = " + std::to_string(c->n_elites) + " outside 2..256");
    if (c->max_trials < 1) return fail(VF_ERR_INVALID, w + ": max_trials = " + std::to_string(c->max_trials) + ", need at least 1");
    if (c->discrete_mask < 0 || c->discrete_mask >= (1 << c->adim))
        return fail(VF_ERR_INVALID, w + ": discrete_mask names a column past adim");
    for (int i = 0; i < c->adim; ++i)
        if (!(c->rej_lim[i] >= 0.0) || !(c->trunc_lim[i] >= 0.0))
            return fail(VF_ERR_INVALID, w + ": rej_lim and trunc_lim must be >= 0 (+inf = none)");
    return VF_OK;
}
static int cem_config_check(const vf_cem_corr_config *c, const char *who) {
    const std::string w(who);
    if (!c) return fail(VF_ERR_INVALID, w + ": null cfg");
    if (c->nactions < 1 || c->adim < 1 || c->tail < 0 || c->adim + c->tail > kCemMaxWidth)
        return fail(VF_ERR_INVALID, w + ": need nactions >= 1, adim >= 1, tail >= 0 and adim + tail <= 8");
    if ((long long)c->nactions * c->adim > kCemMaxD)
        return fail(VF_ERR_INVALID, w + ": D = nactions * adim = " + std::to_string((long long)c->nactions * c->adim) + " exceeds 128");
    const int least = c->refit_cov ? 2 : 1;
    if (c->n_elites < least || c->n_elites > kCemMaxK)
        return fail(VF_ERR_INVALID, w + ": n_elites = " + std::to_string(c->n_elites) + " outside " + std::to_string(least) + "..256");
    return VF_OK;
}

// The clauses the entries repeat, under the entry's name.  All ten: the device and any null pointer among the entry's own ...
static int cem_call_check(const char *who, int32_t device, bool any_null) {
    const std::string w(who);
    if (device < 0) return fail(VF_ERR_INVALID, w + ": device = " + std::to_string(device) + " is negative");
    if (any_null) return fail(VF_ERR_INVALID, w + ": null argument");
    return VF_OK;
}
// ... and the six with a workspace: its alignment and M in least..kCemMaxM (`least_text`: how the message names the bound)
static int cem_workspace_check(const char *who, const void *d_workspace, int32_t M, int least, const char *least_text) {
    const std::string w(who);
    if (reinterpret_cast<uintptr_t>(d_workspace) % 16) return fail(VF_ERR_INVALID, w + ": d_workspace must be 16-byte aligned");
    if (M < least || M > kCemMaxM)
        return fail(VF_ERR_INVALID, w + ": M = " + std::to_string(M) + " outside " + least_text + ".." + std::to_string(kCemMaxM));
    return VF_OK;
}

// the argument refusals of vf_cem_refit / vf_cem_soft_refit, behind the config check of either
static int cem_refit_check(const char *who, int32_t device, int n_elites, const double *d_scores, const float *d_actions, int32_t M,
                           const int32_t *d_elite_index, const double *d_elite_score, const float *d_elite_plans,
                           const void *d_workspace) {
    const bool any_null = !d_scores || !d_actions || !d_elite_index || !d_elite_score || !d_elite_plans || !d_workspace;
    if (int rc = cem_call_check(who, device, any_null)) return rc;
    return cem_workspace_check(who, d_workspace, M, n_elites, "n_elites");
}

#ifndef VF_HOST_SELFTEST
static CemParams cem_params(const vf_cem_config &c, int M) {
    CemParams p = {};
    p.nactions = c.nactions; p.repeat = c.repeat; p.adim = c.adim; p.tail = c.tail;
    p.K = c.n_elites; p.M = M;
    p.max_trials = c.max_trials; p.rejection = c.rejection != 0; p.zero_first = c.zero_first != 0;
    p.discrete_mask = c.discrete_mask;
    p.seed_lo = c.seed_lo; p.seed_hi = c.seed_hi;
    for (int i = 0; i < kCemMaxWidth; ++i) {
        p.rej_lim[i] = c.rej_lim[i]; p.trunc_lim[i] = c.trunc_lim[i]; p.tail_value[i] = c.tail_value[i];
    }
    return p;
}
static CemCorrParams cem_corr_params(const vf_cem_corr_config &c, int M) {
    CemCorrParams p = {};
    p.nactions = c.nactions; p.adim = c.adim; p.tail = c.tail; p.K = c.n_elites; p.M = M;
    p.refit_cov = c.refit_cov != 0; p.has_first_prev = c.has_first_prev != 0;
    p.seed_lo = c.seed_lo; p.seed_hi = c.seed_hi;
    p.kappa = c.kappa; p.beta_0 = c.beta_0; p.beta_1 = c.beta_1;
    for (int i = 0; i < kCemMaxWidth; ++i) {
        p.std[i] = c.std[i]; p.bias[i] = c.bias[i]; p.first_prev[i] = c.first_prev[i]; p.tail_value[i] = c.tail_value[i];
    }
    return p;
}

// `blocks` workgroups of kCemThreads on the caller's stream of `device`, and what the launch reports
template <typename... KA, typename... A>
static int cem_launch(void (*kernel)(KA...), int32_t device, long long blocks, void *stream, A... args) {
    VF_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kCemThreads), 0, reinterpret_cast<hipStream_t>(stream), args...);
    VF_HIP_CHECK(hipGetLastError());
    return VF_OK;
}
// the workgroups of "one wavefront per item" (vf_cem.h: kCemWaves per workgroup)
static long long cem_wave_blocks(int n) { return (n + kCemWaves - 1) / kCemWaves; }
#endif

}  // namespace vf

extern "C" {

size_t vf_cem_workspace_bytes(const vf_cem_config *cfg) {
    VF_API_TRY
    if (cem_config_check(cfg, "vf_cem_workspace_bytes")) return 0;
    return cem_workspace_bytes(cfg->nactions * cfg->adim, cfg->n_elites);
    VF_API_CATCH(size_t)
}

size_t vf_cem_corr_workspace_bytes(const vf_cem_corr_config *cfg) {
    VF_API_TRY
    if (cem_config_check(cfg, "vf_cem_corr_workspace_bytes")) return 0;
    return cem_corr_workspace_bytes(cfg->nactions * cfg->adim, cfg->n_elites, cfg->refit_cov != 0);
    VF_API_CATCH(size_t)
}

int vf_cem_refit(int32_t device, const vf_cem_config *cfg, const double *d_scores, const float *d_actions, int32_t M,
                 int32_t *d_elite_index, double *d_elite_score, float *d_elite_plans, void *d_workspace, void *stream) {
    VF_API_TRY
    if (int rc = cem_config_check(cfg, "vf_cem_refit")) return rc;
    if (int rc = cem_refit_check("vf_cem_refit", device, cfg->n_elites, d_scores, d_actions, M, d_elite_index, d_elite_score,
                                 d_elite_plans, d_workspace))
        return rc;
#ifdef VF_HOST_SELFTEST
    (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemParams p = cem_params(*cfg, M);
    p.scores = d_scores; p.actions_in = d_actions;
    p.elite_index = d_elite_index; p.elite_score = d_elite_score; p.elite_plans = d_elite_plans;
    p.workspace = d_workspace;
    return cem_launch(cem_refit_kernel, device, 1, stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_sample(int32_t device, const vf_cem_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                  float *d_actions, int32_t *d_trials, int32_t *d_capped, void *stream) {
    VF_API_TRY
    if (int rc = cem_config_check(cfg, "vf_cem_sample")) return rc;
    if (int rc = cem_call_check("vf_cem_sample", device, !d_workspace || !d_actions || !d_trials || !d_capped)) return rc;
    if (int rc = cem_workspace_check("vf_cem_sample", d_workspace, M, 1, "1")) return rc;
#ifdef VF_HOST_SELFTEST
    (void)call; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemParams p = cem_params(*cfg, M);
    p.call = call;
    p.actions_out = d_actions; p.trials = d_trials; p.capped = d_capped;
    p.workspace = const_cast<void *>(d_workspace);
    return cem_launch(cem_sample_kernel, device, cem_wave_blocks(M), stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_soft_refit(int32_t device, const vf_cem_corr_config *cfg, const double *d_scores, const float *d_actions, int32_t M,
                      int32_t *d_elite_index, double *d_elite_score, float *d_elite_plans, void *d_workspace, void *stream) {
    VF_API_TRY
    if (int rc = cem_config_check(cfg, "vf_cem_soft_refit")) return rc;
    if (int rc = cem_refit_check("vf_cem_soft_refit", device, cfg->n_elites, d_scores, d_actions, M, d_elite_index, d_elite_score,
                                 d_elite_plans, d_workspace))
        return rc;
#ifdef VF_HOST_SELFTEST
    (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemCorrParams p = cem_corr_params(*cfg, M);
    p.scores = d_scores; p.actions_in = d_actions;
    p.elite_index = d_elite_index; p.elite_score = d_elite_score; p.elite_plans = d_elite_plans;
    p.workspace = d_workspace;
    return cem_launch(cem_soft_refit_kernel, device, 1, stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_sample_corr(int32_t device, const vf_cem_corr_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                       float *d_actions, void *stream) {
    VF_API_TRY
    if (int rc = cem_config_check(cfg, "vf_cem_sample_corr")) return rc;
    if (int rc = cem_call_check("vf_cem_sample_corr", device, !d_workspace || !d_actions)) return rc;
    if (int rc = cem_workspace_check("vf_cem_sample_corr", d_workspace, M, 1, "1")) return rc;
#ifdef VF_HOST_SELFTEST
    (void)call; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemCorrParams p = cem_corr_params(*cfg, M);
    p.call = call;
    p.actions_out = d_actions;
    p.workspace = const_cast<void *>(d_workspace);
    return cem_launch(cem_sample_corr_kernel, device, cem_wave_blocks(M), stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_sample_fold(int32_t device, const vf_cem_fold_config *cfg, const void *d_workspace, uint32_t call, int32_t M,
                       float *d_actions, void *stream) {
    VF_API_TRY
    const std::string w("vf_cem_sample_fold");
    if (!cfg) return fail(VF_ERR_INVALID, w + ": null cfg");
    if (cfg->nactions < kCemFoldSteps || cfg->nactions * kCemFoldAdim > kCemMaxD)
        return fail(VF_ERR_INVALID, w + ": nactions = " + std::to_string(cfg->nactions) + " outside 5..32");
    if (cfg->repeat < 1 || (long long)cfg->nactions * cfg->repeat > (1 << 16))
        return fail(VF_ERR_INVALID, w + ": need repeat >= 1 and T = nactions * repeat <= 2^16");
    if (cfg->tail < 0 || kCemFoldAdim + cfg->tail > kCemMaxWidth) return fail(VF_ERR_INVALID, w + ": tail outside 0..4");
    if (cfg->n_elites < 2 || cfg->n_elites > kCemMaxK)
        return fail(VF_ERR_INVALID, w + ": n_elites = " + std::to_string(cfg->n_elites) + " outside 2..256");
    for (int i = 0; i < 3; ++i)
        if (!(cfg->max_shift[i] >= 0.0)) return fail(VF_ERR_INVALID, w + ": max_shift must be >= 0 (+inf = none)");
    if (int rc = cem_call_check(w.c_str(), device, !d_workspace || !d_actions)) return rc;
    if (int rc = cem_workspace_check(w.c_str(), d_workspace, M, 1, "1")) return rc;
    if (cfg->n_scripted < 1 || 2LL * cfg->n_scripted > M)
        return fail(VF_ERR_INVALID, w + ": n_scripted = " + std::to_string(cfg->n_scripted) + ", need 1 <= 2 * n_scripted <= M = " +
                                        std::to_string(M));
#ifdef VF_HOST_SELFTEST
    (void)call; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemFoldParams p = {};
    p.nactions = cfg->nactions; p.repeat = cfg->repeat; p.tail = cfg->tail; p.K = cfg->n_elites; p.M = M;
    p.n_scripted = cfg->n_scripted;
    p.seed_lo = cfg->seed_lo; p.seed_hi = cfg->seed_hi; p.call = call;
    for (int i = 0; i < 2; ++i) p.start_xy[i] = cfg->start_xy[i];
    for (int i = 0; i < 3; ++i) p.max_shift[i] = cfg->max_shift[i];
    for (int i = 0; i < kCemMaxWidth; ++i) p.tail_value[i] = cfg->tail_value[i];
    p.actions_out = d_actions;
    p.workspace = d_workspace;
    return cem_launch(cem_sample_fold_kernel, device, cem_wave_blocks(M), stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_sample_autograsp(int32_t device, const vf_cem_config *cfg, const vf_cem_grip_config *grip, const void *d_workspace,
                            uint32_t call, int32_t M, const float *d_elite_plans, float *d_share, float *d_actions,
                            int32_t *d_trials, int32_t *d_capped, void *stream) {
    VF_API_TRY
    const std::string w("vf_cem_sample_autograsp");
    if (int rc = cem_config_check(cfg, w.c_str())) return rc;
    if (cfg->adim < kCemGripLift + 1)
        return fail(VF_ERR_INVALID, w + ": adim = " + std::to_string(cfg->adim) + " move channels, the height reads channel 2");
    if (cfg->tail < 1) return fail(VF_ERR_INVALID, w + ": tail = 0 leaves no gripper column behind the moves");
    if (!grip) return fail(VF_ERR_INVALID, w + ": null grip");
    if (grip->mode != kCemGripHeight && grip->mode != kCemGripShare)
        return fail(VF_ERR_INVALID, w + ": mode = " + std::to_string(grip->mode) + " is neither 0 (height) nor 1 (share)");
    if (!(grip->deviation_prob >= 0.0 && grip->deviation_prob <= 1.0))
        return fail(VF_ERR_INVALID, w + ": deviation_prob outside [0, 1]");
    if (int rc = cem_call_check(w.c_str(), device, !d_workspace || !d_actions || !d_trials || !d_capped)) return rc;
    if (grip->mode == kCemGripShare && (!d_elite_plans || !d_share))
        return fail(VF_ERR_INVALID, w + ": share mode needs d_elite_plans and d_share");
    if (int rc = cem_workspace_check(w.c_str(), d_workspace, M, 1, "1")) return rc;
    if (reinterpret_cast<uintptr_t>(d_actions) % 4 || reinterpret_cast<uintptr_t>(d_trials) % 4 ||
        reinterpret_cast<uintptr_t>(d_capped) % 4 || reinterpret_cast<uintptr_t>(d_elite_plans) % 4 ||
        reinterpret_cast<uintptr_t>(d_share) % 4)
        return fail(VF_ERR_INVALID, w + ": d_actions, d_trials, d_capped, d_elite_plans and d_share must be 4-byte aligned");
#ifdef VF_HOST_SELFTEST
    (void)call; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemParams p = cem_params(*cfg, M);
    p.call = call;
    p.actions_out = d_actions; p.trials = d_trials; p.capped = d_capped;
    p.workspace = const_cast<void *>(d_workspace);
    CemGripParams g = {};
    g.mode = grip->mode; g.reopen = grip->reopen != 0;
    g.state_z = grip->state_z; g.norm = grip->action_norm_factor; g.z_thresh = grip->z_thresh;
    g.deviation_prob = grip->deviation_prob;
    g.close_cmd = (float)grip->close_cmd; g.open_cmd = (float)grip->open_cmd;
    if (g.mode == kCemGripShare) {
        g.elite_plans = d_elite_plans; g.share = d_share;
        if (int rc = cem_launch(cem_grip_share_kernel, device, 1, stream, g, cfg->n_elites, cfg->nactions * cfg->repeat,
                                cfg->adim + cfg->tail, cfg->adim))
            return rc;
    }
    return cem_launch(cem_sample_autograsp_kernel, device, cem_wave_blocks(M), stream, p, g);
#endif
    VF_API_CATCH(int)
}

int vf_cem_latents(int32_t device, uint32_t seed_lo, uint32_t seed_hi, uint32_t call, int32_t n_latent, int32_t T,
                   int32_t zdim, float *d_z, void *stream) {
    VF_API_TRY
    const std::string w("vf_cem_latents");
    if (n_latent < 1) return fail(VF_ERR_INVALID, w + ": n_latent = " + std::to_string(n_latent) + ", need at least 1");
    if (T < 1) return fail(VF_ERR_INVALID, w + ": T = " + std::to_string(T) + ", need at least 1");
    if (zdim < 1) return fail(VF_ERR_INVALID, w + ": zdim = " + std::to_string(zdim) + ", need at least 1");
    if ((long long)T * zdim > (1LL << 30))
        return fail(VF_ERR_INVALID, w + ": T * zdim = " + std::to_string((long long)T * zdim) + " exceeds 2^30");
    if (int rc = cem_call_check(w.c_str(), device, !d_z)) return rc;
    if (reinterpret_cast<uintptr_t>(d_z) % 4) return fail(VF_ERR_INVALID, w + ": d_z must be 4-byte aligned");
#ifdef VF_HOST_SELFTEST
    (void)seed_lo; (void)seed_hi; (void)call; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    CemLatentParams p = {};
    p.n_latent = n_latent;
    p.N = (long long)T * zdim;
    p.n_blocks = (int)((p.N + 3) / 4);
    p.seed_lo = seed_lo; p.seed_hi = seed_hi; p.call = call;
    p.z = d_z;
    return cem_launch(cem_latents_kernel, device, cem_wave_blocks(n_latent), stream, p);
#endif
    VF_API_CATCH(int)
}

int vf_cem_fold_latents(int32_t device, const float *d_actions, const float *d_z, int32_t M, int32_t n_latent, int32_t T,
                        int32_t width, int32_t zdim, float *d_seqs, void *stream) {
    VF_API_TRY
    const std::string w("vf_cem_fold_latents");
    if (M < 1) return fail(VF_ERR_INVALID, w + ": M = " + std::to_string(M) + ", need at least 1");
    if (n_latent < 1) return fail(VF_ERR_INVALID, w + ": n_latent = " + std::to_string(n_latent) + ", need at least 1");
    if (T < 1) return fail(VF_ERR_INVALID, w + ": T = " + std::to_string(T) + ", need at least 1");
    if (width < 1) return fail(VF_ERR_INVALID, w + ": width = " + std::to_string(width) + ", need at least 1");
    if (zdim < 1) return fail(VF_ERR_INVALID, w + ": zdim = " + std::to_string(zdim) + ", need at least 1");
    if ((long long)M * n_latent > INT32_MAX)
        return fail(VF_ERR_INVALID, w + ": M * n_latent = " + std::to_string((long long)M * n_latent) + " rows do not fit in int32");
    if ((long long)T * ((long long)width + zdim) > INT32_MAX)
        return fail(VF_ERR_INVALID, w + ": T * (width + zdim) = " + std::to_string((long long)T * ((long long)width + zdim)) +
                                        " floats per row do not fit in int32");
    if (int rc = cem_call_check(w.c_str(), device, !d_actions || !d_z || !d_seqs)) return rc;
    if (reinterpret_cast<uintptr_t>(d_actions) % 4 || reinterpret_cast<uintptr_t>(d_z) % 4 ||
        reinterpret_cast<uintptr_t>(d_seqs) % 4)
        return fail(VF_ERR_INVALID, w + ": d_actions, d_z and d_seqs must be 4-byte aligned");
#ifdef VF_HOST_SELFTEST
    (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    // float4s where every piece of a row starts on a 16-byte boundary
    const bool vec = width % 4 == 0 && zdim % 4 == 0 && reinterpret_cast<uintptr_t>(d_actions) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(d_z) % 16 == 0 && reinterpret_cast<uintptr_t>(d_seqs) % 16 == 0;
    CemFoldLatentParams p = {};
    p.n_latent = n_latent; p.T = T; p.width = width; p.zdim = zdim;
    p.total = (long long)M * n_latent * T * (((long long)width + zdim) / (vec ? 4 : 1));
    p.actions = d_actions; p.z = d_z; p.seqs = d_seqs;
    const long long blocks = std::min<long long>((p.total + kCemThreads - 1) / kCemThreads, kCemFoldMaxBlocks);
    return cem_launch(vec ? cem_fold_latents_kernel<true> : cem_fold_latents_kernel<false>, device, blocks, stream, p);
#endif
    VF_API_CATCH(int)
}

}  // extern "C"
