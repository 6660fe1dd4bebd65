// vf_engine_invmodel.inc - host side of the action-inference network (vf_inverse_model.h; include/vf_hip.h "Inverse-model
// policy"): tensor table, buffers, the launch sequence.  Included at the end of vf_engine.hip, after the other side
// networks and vf_engine_sidenet.inc (allocation, upload, weight packing, also under -DVF_HOST_SELFTEST).

struct vf_invmodel {
    vf_invmodel_config cfg;
    int H = 0, W = 0, adim = 0, n_context = 0, n_actions = 0;
    int n_img = 0;                                      // max_batch * (1 + n_context)
    float *w1[2] = {nullptr}, *b1[2] = {nullptr};       // c1 of the pair / ctx tower as in the blob, [9 * cin * 32], [32]
    float *wp[3] = {nullptr}, *b[3] = {nullptr};        // c2 .. c4 packed for vf_net_conv.h [2][packed], biases [2][Cout]
    float *wx = nullptr, *wa = nullptr, *wh = nullptr, *bl = nullptr;      // the cell: [128][512], [adim][512], [128][512], [512]
    float *wo = nullptr, *bo = nullptr;                 // [128][adim], [adim]
    float *act[4] = {nullptr};                          // outputs of c1 .. c4 for n_img images
    float *pre = nullptr;                               // [n_img][512] input parts of the gate sums
    bool loaded = false;
    std::vector<AllocRec> allocs;
};

namespace vf {

static const int kImTowerCin[2] = {6, 3};               // pair, ctx

static int invmodel_validate(const vf_invmodel_config *cfg) {
    if (!cfg) return fail(VF_ERR_INVALID, "null inverse-model config");
    if (cfg->height < 16 || cfg->width < 16 || cfg->height % 16 || cfg->width % 16)
        return fail(VF_ERR_INVALID, "inverse-model height and width must be multiples of 16");
    if (cfg->width > 128)
        return fail(VF_ERR_INVALID, "inverse-model width must be at most 128 (the staged rows of c1 stay within 64 KiB of LDS)");
    if (cfg->adim < 1 || cfg->adim > kImMaxAdim) return fail(VF_ERR_INVALID, "inverse-model adim must be 1..8");
    if (cfg->n_context < 1 || cfg->n_context > kImMaxContext) return fail(VF_ERR_INVALID, "inverse-model n_context must be 1..4");
    if (cfg->n_actions < 1 || cfg->n_actions > 32) return fail(VF_ERR_INVALID, "inverse-model n_actions must be 1..32");
    if (cfg->max_batch < 1 || cfg->max_batch > 4096) return fail(VF_ERR_INVALID, "inverse-model max_batch must be 1..4096");
    if (!(cfg->input_scale > 0.f)) return fail(VF_ERR_INVALID, "inverse-model input_scale must be positive");
    return VF_OK;
}

static size_t invmodel_blob_floats(int adim) {
    size_t n = 0;
    for (int tw = 0; tw < 2; ++tw) {
        int c_in = kImTowerCin[tw];
        for (int l = 1; l <= 4; ++l) { n += (size_t)9 * c_in * kScCh[l] + kScCh[l]; c_in = kScCh[l]; }
    }
    return n + (size_t)(2 * kImUnits + adim) * kImGates + kImGates + (size_t)kImUnits * adim + adim;
}

// the refusals of vf_invmodel_infer (host work only: shared by the device build and the host self-test)
static int invmodel_infer_check(const vf_invmodel *m, const float *d_start, const float *d_goal, const float *d_ctx_frames,
                                const float *d_ctx_actions, int32_t n, const float *d_actions) {
    if (!m || !d_start || !d_goal || !d_ctx_frames || !d_ctx_actions || !d_actions) return fail(VF_ERR_INVALID, "null argument");
    if (!m->loaded) return fail(VF_ERR_INVALID, "inverse-model weights not loaded");
    if (n < 1 || n > m->cfg.max_batch)
        return fail(VF_ERR_INVALID, "n = " + std::to_string(n) + " problems, max_batch = " + std::to_string(m->cfg.max_batch));
    if (reinterpret_cast<uintptr_t>(d_start) % 16 || reinterpret_cast<uintptr_t>(d_goal) % 16 ||
        reinterpret_cast<uintptr_t>(d_ctx_frames) % 16)
        return fail(VF_ERR_INVALID, "the images must be 16-byte aligned");
    return VF_OK;
}

#ifndef VF_HOST_SELFTEST
static int invmodel_run(vf_invmodel *m, const float *d_start, const float *d_goal, const float *d_ctx_frames,
                        const float *d_ctx_actions, int n, float *d_actions, float *d_hidden, hipStream_t st) {
    const int H = m->H, W = m->W, n_img = n * (1 + m->n_context);
    const InvModelSrc src = {d_start, d_goal, d_ctx_frames, n, m->n_context};
    const size_t lds = ((size_t)2 * (2 * kImBand + 1) * W * 3 + (size_t)9 * 6 * kScCh[1]) * sizeof(float);
    hipLaunchKernelGGL(invmodel_c1_kernel, dim3((unsigned)(n_img * (H / 2 / kImBand))), dim3(kImThreads), lds, st, src, H, W,
                       m->cfg.input_scale, m->w1[0], m->b1[0], m->w1[1], m->b1[1], m->act[0]);
    VF_HIP_CHECK(hipGetLastError());
    for (int l = 2; l <= 4; ++l) {
        const int Hin = H >> (l - 1), Win = W >> (l - 1), Cin = kScCh[l - 1], Cout = kScCh[l];
        const int P = (Hin / 2) * (Win / 2), mtiles = (P + 31) / 32;
        const long long stride = (long long)packed_floats(Cin, Cout);
        if (l == 2)             // NT = 2: all 64 output channels in one wave
            launch_net_conv(invmodel_conv_kernel<2>, n_img, mtiles, 1, st, m->act[0], n_img, n, Hin, Win, Cin, Cout, m->wp[0],
                            m->b[0], stride, m->act[1]);
        else                    // NT = 1: four waves share a row tile (few positions are left, more tasks keep the CUs busy)
            launch_net_conv(invmodel_conv_kernel<1>, n_img, mtiles, Cout / 32, st, m->act[l - 2], n_img, n, Hin, Win, Cin, Cout,
                            m->wp[l - 2], m->b[l - 2], stride, m->act[l - 1]);
        VF_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(invmodel_gates_kernel, dim3((unsigned)n_img), dim3(kImGates), 0, st, m->act[3], (H / 16) * (W / 16), m->wx,
                       m->bl, m->pre);
    VF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(invmodel_lstm_kernel, dim3((unsigned)n), dim3(kImGates), 0, st, m->pre, d_ctx_actions, n, m->adim,
                       m->n_context, m->n_actions, m->wa, m->wh, m->wo, m->bo, d_actions, d_hidden);
    VF_HIP_CHECK(hipGetLastError());
    return VF_OK;
}
#endif

}  // namespace vf

extern "C" {

size_t vf_invmodel_weight_count(const vf_invmodel_config *cfg) {
    VF_API_TRY
    if (invmodel_validate(cfg)) return 0;
    return invmodel_blob_floats(cfg->adim);
    VF_API_CATCH(size_t)
}

int vf_invmodel_destroy(vf_invmodel *m) {
    VF_API_TRY
    if (!m) return VF_OK;
    side_free_all(m->cfg.device, m->allocs);
    delete m;
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_invmodel_create(const vf_invmodel_config *cfg, vf_invmodel **out) {
    vf_invmodel *made = nullptr;     // (released if anything below throws)
    VF_API_TRY
    if (!out) return fail(VF_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int rc = invmodel_validate(cfg);
    if (rc) return rc;
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(cfg->device));
#endif
    vf_invmodel *m = new vf_invmodel();
    made = m;
    m->cfg = *cfg;
    m->H = cfg->height; m->W = cfg->width; m->adim = cfg->adim;
    m->n_context = cfg->n_context; m->n_actions = cfg->n_actions;
    m->n_img = cfg->max_batch * (1 + cfg->n_context);
    for (int tw = 0; tw < 2; ++tw) {
        VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->w1[tw], (size_t)9 * kImTowerCin[tw] * kScCh[1]);
        VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->b1[tw], (size_t)kScCh[1]);
    }
    for (int l = 2; l <= 4; ++l) {
        VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->wp[l - 2], 2 * packed_floats(kScCh[l - 1], kScCh[l]));
        VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->b[l - 2], (size_t)2 * kScCh[l]);
    }
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->wx, (size_t)kImUnits * kImGates);
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->wa, (size_t)m->adim * kImGates);
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->wh, (size_t)kImUnits * kImGates);
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->bl, (size_t)kImGates);
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->wo, (size_t)kImUnits * m->adim);
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->bo, (size_t)m->adim);
    for (int l = 1; l <= 4; ++l)
        VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->act[l - 1], (size_t)m->n_img * scorer_act_floats(m->H, m->W, l));
    VF_SIDE_ALLOC(m, vf_invmodel_destroy, m->pre, (size_t)m->n_img * kImGates);
    *out = m;
    return VF_OK;
    VF_API_CATCH_CLEANUP(int, { if (made) vf_invmodel_destroy(made); if (out) *out = nullptr; })
}

int vf_invmodel_load_weights(vf_invmodel *m, const float *host_blob, size_t n_floats) {
    VF_API_TRY
    if (!m || !host_blob) return fail(VF_ERR_INVALID, "null inverse model or blob");
    const size_t want = invmodel_blob_floats(m->adim);
    if (n_floats != want)
        return fail(VF_ERR_INVALID, "inverse-model weight blob has " + std::to_string(n_floats) + " floats, expected " +
                                        std::to_string(want));
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(m->cfg.device));
    VF_HIP_CHECK(hipDeviceSynchronize());       // (hot swap: calls in flight have finished)
#endif
    BlobCursor blob{host_blob, 0};
    for (int tw = 0; tw < 2; ++tw) {
        blob.view = 0;                          // (c1 has a buffer per tower: the towers differ in their input channels)
        blob.upload(m->w1[tw], (size_t)9 * kImTowerCin[tw] * kScCh[1]);
        blob.upload(m->b1[tw], kScCh[1]);
        blob.view = tw;                         // c2 .. c4: the tower's half of the layer's buffer
        for (int l = 2; l <= 4; ++l) {
            blob.upload_packed(m->wp[l - 2], kScCh[l - 1], kScCh[l]);
            blob.upload(m->b[l - 2], kScCh[l]);
        }
    }
    blob.view = 0;
    blob.upload(m->wx, (size_t)kImUnits * kImGates);
    blob.upload(m->wa, (size_t)m->adim * kImGates);
    blob.upload(m->wh, (size_t)kImUnits * kImGates);
    blob.upload(m->bl, kImGates);
    blob.upload(m->wo, (size_t)kImUnits * m->adim);
    blob.upload(m->bo, m->adim);
    if (blob.rc) return blob.rc;
    m->loaded = true;
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_invmodel_infer(vf_invmodel *m, const float *d_start, const float *d_goal, const float *d_ctx_frames,
                      const float *d_ctx_actions, int32_t n, float *d_actions, float *d_hidden, void *stream) {
    VF_API_TRY
    if (int rc = invmodel_infer_check(m, d_start, d_goal, d_ctx_frames, d_ctx_actions, n, d_actions)) return rc;
#ifdef VF_HOST_SELFTEST
    (void)d_hidden; (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    VF_HIP_CHECK(hipSetDevice(m->cfg.device));
    return invmodel_run(m, d_start, d_goal, d_ctx_frames, d_ctx_actions, n, d_actions, d_hidden, reinterpret_cast<hipStream_t>(stream));
#endif
    VF_API_CATCH(int)
}

}  // extern "C"
